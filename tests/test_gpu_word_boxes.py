"""Word boxes (rt_config.rec_return_word_box) on the MI355X: k_word_boxes inside the pipeline against the numpy restatement
(word_box_ref.py), fed teacher-forced by the oracle session running the HIP workers."""
import ctypes as C
import math

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib, synth, workload
from oracle import ref_lib as R
import word_box_ref as WR

pytestmark = pytest.mark.gpu


def _mixed_dict() -> bytes:
    """6623 entries cycling ASCII letters, digits, ".", "-", punctuation and CJK, so the synthetic rec net's tokens mix
    every raw class"""
    pool = (list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ") + list("0123456789") + [".", "-", ".", "-"] +
            list("!?,;:()/") + ["。", "，"])
    ents, cjk = [], 0
    for i in range(6623):
        if i % 3 == 2:
            ents.append(chr(0x4E00 + cjk)); cjk += 1
        else:
            ents.append(pool[i % len(pool)])
    return ("\n".join(ents) + "\n").encode("utf-8")


DICT = _mixed_dict()


def _cfg(words: bool, **kw):
    cfg = retto_amd.synthetic_session_config(0, **kw)
    cfg.rec_processor_config.character_source = retto_amd.RettoWorkerModelSource.Blob(DICT)
    cfg.rec_processor_config.return_word_box = words
    return cfg


@pytest.fixture(scope="module")
def on_session():
    s = retto_amd.RettoSession(_cfg(True))
    yield s
    s.close()


@pytest.fixture(scope="module")
def off_session():
    s = retto_amd.RettoSession(_cfg(False))
    yield s
    s.close()


@pytest.fixture(scope="module")
def full_dict():
    return retto_amd.parse_dictionary(DICT)


def _planted_for(page_h, page_w, lines, seed):
    page, rects = workload.planted_page(page_h, page_w, lines, seed)
    plan = R.resize_both_plan(page_h, page_w)
    ah, aw = plan[-1] if plan else (page_h, page_w)
    dh, dw = R.resize_either_dims(ah, aw)
    return page, workload.planted_map(dh, dw, page_h, page_w, rects)


def _tall_page():
    """test_extreme_line_shapes' page with one more tall line: h / w >= 1.5 (crops rotated by 270 degrees) beside ordinary
    lines and the widest line of that test"""
    h, w = 400, 1984
    page = np.zeros((h, w, 3), np.uint8)
    rng = np.random.default_rng(3)
    rects = [(20, 30, 1930, 55), (40, 120, 300, 126), (600, 100, 640, 380), (700, 90, 760, 330), (900, 200, 1500, 240)]
    for x0, y0, x1, y1 in rects:
        page[y0:y1, x0:x1] = rng.integers(100, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    plan = R.resize_both_plan(h, w)
    ah, aw = plan[-1] if plan else (h, w)
    dh, dw = R.resize_either_dims(ah, aw)
    return page, workload.planted_map(dh, dw, h, w, rects, shrink=0.05)


def _oracle(session):
    """the oracle session over the test dictionary, running the HIP workers; rec_worker records the probability rows"""
    from oracle.pipeline import OracleSession
    det, cls, rec, _ = synth.synth_models(0)
    o = OracleSession(det, cls, rec, DICT)
    o.det_worker, o.cls_worker = session.worker.det, session.worker.cls
    o.calls = []

    def rec_worker(t):
        p = session.worker.rec(t)
        o.calls.append(p)
        return p
    o.rec_worker = rec_worker
    return o


def _expected_words(o, page, m, r, cls_thresh=np.float32(0.9)):
    """per line: the restatement's words from the oracle's intermediates and the recorded probability rows"""
    o.calls = []
    res = o.run(page, det_map_override=m)
    n = len(res.crops)
    dims = [c.shape[:2] for c in res.crops]
    order = sorted(range(n), key=lambda i: -(float(dims[i][0]) / float(dims[i][1])))
    probs = [None] * n
    for b, p in enumerate(o.calls):
        for j, i in enumerate(order[6 * b:6 * b + 6]):
            probs[i] = p[j]
    ori_h, ori_w = page.shape[:2]
    plan = R.resize_both_plan(ori_h, ori_w)
    after_h, after_w = plan[-1] if plan else (ori_h, ori_w)
    raw_of_id = [WR.raw_class(e) for e in o.dict]
    out = []
    assert len(r.rec_result) == n
    for i in range(n):
        ids, cols = WR.kept_columns(np.argmax(probs[i], axis=-1))
        assert ids == [int(t) for t in r.rec_result[i].tokens], f"line {i}: kept tokens differ"
        T, W = probs[i].shape[0], res.rec_widths[i]
        ch, cw = dims[i]
        resized_w = min(int(math.ceil(48.0 * cw / ch)), W)
        c = r.cls_result[i].label
        rot180 = c.label == 180 and np.float32(c.score) >= cls_thresh
        out.append(WR.line_words(raw_of_id, ids, cols, T, W, resized_w, res.boxes_after[i], rot180, after_w, after_h,
                                 ori_w, ori_h))
    return out, raw_of_id


def _assert_words(r, want, raw_of_id, full_dict):
    n_words = 0
    for k, (g, w) in enumerate(zip(r.rec_result, want)):
        assert g.words is not None
        assert len(g.words) == len(w), f"line {k}"
        for x, d in zip(g.words, w):
            q = x.box.as_array().reshape(8)
            assert np.array_equal(q.view(np.uint32), d["quad"].view(np.uint32)), (k, q, d["quad"])
            assert (x.first_token, x.n_tokens, x.first_col, x.last_col) == \
                (d["first_token"], d["n_tokens"], d["first_col"], d["last_col"])
            assert x.kind == ("cjk" if d["kind"] == WR.KIND_CJK else "alnum")
            assert x.text == "".join(full_dict[int(t)] for t in g.tokens[x.first_token:x.first_token + x.n_tokens])
        assert "".join(x.text for x in g.words) == WR.split_free_text(full_dict, g.tokens, raw_of_id)
        n_words += len(g.words)
    return n_words


def _teacher_forced(session, pages, maps, full_dict, o=None, cls_thresh=np.float32(0.9)):
    res = session.run_batch(pages, det_map_override=maps)
    o = o or _oracle(session)
    total = 0
    kinds = set()
    for page, m, r in zip(pages, maps, res):
        want, raw_of_id = _expected_words(o, page, m, r, cls_thresh)
        total += _assert_words(r, want, raw_of_id, full_dict)
        kinds |= {x.kind for g in r.rec_result for x in g.words}
    return res, total, kinds


# ---------------------------------------------------------------- default off: nothing changes
def test_default_off_changes_nothing(on_session, off_session):
    pages, maps = zip(*[_planted_for(960, 960, 32, s) for s in (101, 102)])
    a = on_session.run_batch(list(pages), det_map_override=list(maps))
    b = off_session.run_batch(list(pages), det_map_override=list(maps))
    assert on_session.last_det_checksum == off_session.last_det_checksum
    for x, y in zip(a, b):
        assert np.array_equal(np.stack([d.boxes.as_array() for d in x.det_result]), np.stack([d.boxes.as_array() for d in y.det_result]))
        assert np.array_equal(np.array([d.score for d in x.det_result], np.float32), np.array([d.score for d in y.det_result], np.float32))
        assert [(c.label.label, c.label.score) for c in x.cls_result] == [(c.label.label, c.label.score) for c in y.cls_result]
        for g, h in zip(x.rec_result, y.rec_result):
            assert np.array_equal(g.tokens, h.tokens) and g.text == h.text
            assert np.array_equal(np.float32(g.score).view(np.uint32), np.float32(h.score).view(np.uint32))
            assert g.words is not None and h.words is None
    # the off session's results carry no words at the C level either
    lib = _lib.load()
    r = off_session.run_batch_raw([pages[0]], [960], [960], det_map_override=[maps[0]])
    try:
        wp = C.POINTER(_lib.Word)()
        assert lib.rt_results_count(r, 0) > 0
        assert lib.rt_results_rec_words(r, 0, 0, C.byref(wp)) == 0
        assert lib.rt_results_rec_word_text(r, 0, 0, 0) is None
    finally:
        lib.rt_results_free(r)


# ---------------------------------------------------------------- teacher-forced against the restatement
def test_c3_pages_teacher_forced(on_session, full_dict):
    pages, maps = zip(*[_planted_for(960, 960, 32, s) for s in (201, 202, 203)])
    _, total, kinds = _teacher_forced(on_session, list(pages), list(maps), full_dict)
    assert total > 50 and kinds == {"cjk", "alnum"}


def test_shrunk_page_teacher_forced(on_session, full_dict):
    """resize_both shrinks the page: word quads are scaled back to the original image like the line boxes"""
    page, m = _planted_for(2100, 1500, 7, 43)
    assert R.resize_both_plan(2100, 1500)
    _, total, _ = _teacher_forced(on_session, [page], [m], full_dict)
    assert total > 0


def test_tall_and_widest_lines_teacher_forced(on_session, full_dict):
    page, m = _tall_page()
    res, total, _ = _teacher_forced(on_session, [page], [m], full_dict)
    assert total > 0
    o = _oracle(on_session)
    r = o.run(page, det_map_override=m)
    assert any(WR.crop_geometry(b)[2] for b in r.boxes_after), "no rotate270 line"
    assert max(r.rec_widths) >= 1500   # the widest line: over 190 time steps, several 64-step ballot chunks


def test_rot180_lines_teacher_forced(models, full_dict):
    """the flipped-head classifier of test_pipeline_cls_rotation: rotate180 lines map their words back reversed"""
    import types
    t = synth.cls_tensors(3)
    t["cls.head.fc.w"] = -t["cls.head.fc.w"] * 4; t["cls.head.fc.b"] = -t["cls.head.fc.b"]
    cls_blob = synth.pack_blob(t)
    cfg = _cfg(True)
    cfg.worker_config.models.cls = retto_amd.RettoWorkerModelSource.Blob(cls_blob)
    cfg.cls_processor_config.thresh = 0.55
    s = retto_amd.RettoSession(cfg)
    try:
        o = _oracle(s)

        def cls_process(self, crops, dims):
            n = len(crops)
            lab = np.zeros(n, np.uint16); sc = np.zeros(n, np.float32)
            order = sorted(range(n), key=lambda i: -(float(dims[i][0]) / float(dims[i][1])))
            for s0 in range(0, n, 6):
                idxs = order[s0:s0 + 6]
                tt = np.stack([R.resize_norm_image(crops[i], dims[i][0], dims[i][1], 48, 192, 0.0) for i in idxs])
                idx, scs = R.cls_postprocess(self.cls_worker(tt))
                for j, i in enumerate(idxs):
                    l = [0, 180][int(idx[j])]
                    if l == 180 and scs[j] >= np.float32(0.55):
                        crops[i] = R.rotate180(crops[i])
                    lab[i] = l; sc[i] = scs[j]
            return lab, sc
        o.cls_process = types.MethodType(cls_process, o)
        page, m = _planted_for(480, 640, 6, 31)
        res, total, _ = _teacher_forced(s, [page], [m], full_dict, o=o, cls_thresh=np.float32(0.55))
        assert total > 0
        assert any(c.label.label == 180 and np.float32(c.label.score) >= np.float32(0.55) and g.words
                   for c, g in zip(res[0].cls_result, res[0].rec_result))
    finally:
        s.close()


# ---------------------------------------------------------------- every entry point shares the lane job
def _words_of(res):
    return [[(x.text, x.kind, tuple(x.box.as_array().reshape(8).tolist()), x.first_token, x.n_tokens, x.first_col, x.last_col)
             for x in g.words] for r in res for g in r.rec_result]


def test_submit_wait_equals_run_batch(on_session):
    pages, maps = zip(*[_planted_for(960, 960, 32, s) for s in (301, 302, 303, 304)])
    pages, maps = list(pages), list(maps)
    a = on_session.run_batch(pages, det_map_override=maps)
    t1 = on_session.submit_batch_raw(pages, [960] * 4, [960] * 4, det_map_override=maps)
    t2 = on_session.submit_batch_raw(pages[::-1], [960] * 4, [960] * 4, det_map_override=maps[::-1])
    outs = []
    for t in (t1, t2):
        r = on_session.wait_batch_raw(t)
        try:
            outs.append([on_session._collect(r, i) for i in range(4)])
        finally:
            on_session._hd.lib.rt_results_free(r)
    assert _words_of(outs[0]) == _words_of(a)
    assert _words_of(outs[1]) == _words_of(a[::-1])
    assert sum(len(g.words) for r in a for g in r.rec_result) > 0


def test_fp16_server_session():
    """the PP-OCRv4 server graphs in fp16: same tokens and text with the option on and off; words consistent with them"""
    full = retto_amd.parse_dictionary(DICT)
    raw_of_id = [WR.raw_class(e) for e in full]
    pages, maps = zip(*[_planted_for(960, 960, 16, s) for s in (401, 402)])
    outs = []
    for on in (True, False):
        s = retto_amd.RettoSession(_cfg(on, server=True, dtype="f16"))
        try:
            outs.append(s.run_batch(list(pages), det_map_override=list(maps)))
        finally:
            s.close()
    total = 0
    for r, q, page in zip(outs[0], outs[1], pages):
        H, W = page.shape[:2]
        for g, h in zip(r.rec_result, q.rec_result):
            assert np.array_equal(g.tokens, h.tokens) and g.text == h.text and h.words is None
            assert "".join(x.text for x in g.words) == WR.split_free_text(full, g.tokens, raw_of_id)
            cols = [x.first_col for x in g.words]
            assert cols == sorted(cols) and all(x.first_col <= x.last_col for x in g.words)
            for x in g.words:
                b = x.box.as_array()
                assert (b[:, 0] >= 0).all() and (b[:, 0] <= W - 1).all() and (b[:, 1] >= 0).all() and (b[:, 1] <= H - 1).all()
            total += len(g.words)
    assert total > 0


def test_rt_create_rejects_other_values():
    c = _lib.Config()
    lib = _lib.load()
    lib.rt_config_default(C.byref(c))
    c.rec_return_word_box = 2
    h = C.c_void_p()
    assert lib.rt_create(C.byref(c), C.byref(h)) == retto_amd.InvalidArgument.code
    assert b"rec_return_word_box" in lib.rt_last_error(None)

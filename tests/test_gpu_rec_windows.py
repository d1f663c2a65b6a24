"""Rec windows (retto_amd/csrc/rec_windows.h) on the GPU: the stitch against the numpy selection of rec_windows_ref byte for
byte, every unit's rows against the fp32 oracle on the numpy-cut unit, whole lines and windows-off runs untouched, the pipeline
(rt_run_regions) against the debug entry fed with the rebuilt line tensors, the rec options riding along, and the setter's guard.

Bounds of the oracle comparison are test_rec_net's (tests/test_gpu_parity.py): |prob - max(ref)| <= 2e-4, idx == argmax(ref)
wherever the oracle's top-2 margin exceeds 1e-4, decisive rows more than 0.9 of all rows over the test."""
import numpy as np
import pytest
import torch

from oracle import nets_torch as N
import retto_amd

import rec_windows_ref as WR

pytestmark = pytest.mark.gpu

REC_ATOL, REC_MARGIN, DECISIVE_FLOOR = 2e-4, 1e-4, 0.9
CASES = [(487, 128, 32), (330, 128, 64), (656, 256, 64), (200, 128, 0)]
CASE_UNITS = [5, 5, 4, 2]
WHOLE = 120


def _line(L, seed):
    """uniform(-1, 1), seeded, the last fifth of the columns zeroed (right-hand padding like resize_norm_image)"""
    x = np.random.default_rng(seed).uniform(-1, 1, (3, 48, L)).astype(np.float32)
    x[:, :, L - L // 5:] = 0.0
    return x


def _rand_page(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _session(**kw):
    return retto_amd.RettoSession(retto_amd.synthetic_session_config(0, **kw))


@pytest.fixture(scope="module")
def s32():
    s = _session(lanes=1)
    yield s
    s.close()


def _debug_case(s, k, seed0):
    """one debug_rec_windows call under case k's setting: the case's line with the whole line alongside, as ONE group"""
    L, W, O = CASES[k]
    lines = [_line(L, seed0 + k), _line(WHOLE, seed0 + 50 + k)]
    s.set_rec_windows(W, O)
    assert s.rec_windows == (W, O)
    try:
        return (lines,) + s.debug_rec_windows(lines)
    finally:
        s.set_rec_windows(0)


@pytest.fixture(scope="module")
def window_runs(s32):
    """every case on the fp32 session, computed once"""
    return [_debug_case(s32, k, 700) for k in range(len(CASES))]


def _calls(prof, name):
    return prof.get(name, (0.0, 0))[1]


def _assert_selection(k, lines, units, stitched, plans):
    L, W, O = CASES[k]
    assert plans[0] == WR.as_dict(L, W, O) and plans[1] == WR.as_dict(WHOLE, W, O)
    assert [len(u) for u in units] == [CASE_UNITS[k], 1]
    for us, st, p in zip(units, stitched, plans):
        for j, (idx, prob, z5) in enumerate(us):
            assert len(idx) == len(prob) == len(z5) == WR.tokens(p["widths"][j]) and z5.shape[1] == 120
            assert np.isfinite(prob).all() and np.isfinite(z5).all()
        for a in range(3):   # idx, prob, z5 rows alike
            want = WR.stitch([u[a] for u in us], p["origins"], p["bounds"], p["T"])
            assert st[a].shape == want.shape and st[a].tobytes() == want.tobytes(), (k, a)
        assert np.isfinite(st[1]).all() and np.isfinite(st[2]).all()
    # the whole line is one unit that owns all its rows
    assert all(units[1][0][a].tobytes() == stitched[1][a].tobytes() for a in range(3))


# ---- 1. the stitch is a selection ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=["%d-%d-%d" % c for c in CASES])
def test_stitch_is_a_selection(window_runs, k):
    _assert_selection(k, *window_runs[k])


def test_stitch_is_a_selection_f16():
    s = _session(lanes=1, dtype="f16")
    try:
        _assert_selection(0, *_debug_case(s, 0, 800))
    finally:
        s.close()


# ---- 2. every unit against the oracle on the cut unit ------------------------------------------------------------------------
def test_units_equal_the_oracle_on_the_cut_unit(window_runs, oracle_session):
    rows = decisive_n = 0
    worst = 0.0
    for k, (lines, units, stitched, plans) in enumerate(window_runs):
        for x, us, p in zip(lines, units, plans):
            for j, (idx, prob, z5) in enumerate(us):
                x0, w = p["origins"][j], p["widths"][j]
                cut = np.ascontiguousarray(x[None, :, :, x0:x0 + w])
                ref = N.rec_forward(oracle_session.wr, torch.from_numpy(cut)).numpy()[0]
                assert ref.shape[0] == len(idx)
                err = float(np.abs(prob - ref.max(-1)).max())
                top2 = np.sort(ref, -1)[..., -2:]
                decisive = (top2[..., 1] - top2[..., 0]) > REC_MARGIN
                print("case %d unit %d (x0 %d, w %d): max abs err %.3e, decisive %d / %d" % (k, j, x0, w, err, decisive.sum(), decisive.size))
                assert err <= REC_ATOL, (k, j, err)
                assert (idx[decisive] == ref.argmax(-1)[decisive]).all(), (k, j)
                rows += decisive.size; decisive_n += int(decisive.sum()); worst = max(worst, err)
    print("units: worst max abs err %.3e, decisive share %.4f of %d rows" % (worst, decisive_n / rows, rows))
    assert decisive_n > DECISIVE_FLOOR * rows, (decisive_n, rows)


# ---- the pages of tests 3 - 6: regions of known size on noise pages -----------------------------------------------------------
def _rect(x0, y0, w, h):
    return [x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h]


REGION_PAGES = [((64, 1340), [_rect(12, 8, 1300, 48)]), ((64, 740), [_rect(16, 6, 700, 48)]),
                ((120, 460), [_rect(10, 8, 400, 40), _rect(20, 70, 200, 30)])]
REGION_UNITS = [[5], [3], [2, 2]]   # rec widths 1300, 700 and 480 / 480 (the page's batch width) under windows 320 / 64


def _region_pages(seed):
    return [_rand_page(h, w, seed + i) for i, ((h, w), _) in enumerate(REGION_PAGES)], [q for _, q in REGION_PAGES]


def _same(a, b):
    """two RettoWorkerResults of calls with the same pages equal bit for bit, as _same of test_gpu_det_tiles.py"""
    assert len(a.det_result) == len(b.det_result)
    for x, y in zip(a.det_result, b.det_result):
        assert np.array_equal(x.boxes.as_array(), y.boxes.as_array())
        assert np.float32(x.score).tobytes() == np.float32(y.score).tobytes()
    assert [c.label.label for c in a.cls_result] == [c.label.label for c in b.cls_result]
    assert [np.float32(c.label.score).tobytes() for c in a.cls_result] == [np.float32(c.label.score).tobytes() for c in b.cls_result]
    for x, y in zip(a.rec_result, b.rec_result):
        assert np.array_equal(x.tokens, y.tokens) and x.text == y.text
    assert [np.float32(x.score).tobytes() for x in a.rec_result] == [np.float32(y.score).tobytes() for y in b.rec_result]


# ---- 3. off and whole lines are untouched --------------------------------------------------------------------------------------
def test_whole_lines_and_windows_off_launch_nothing_new():
    from oracle import ref_lib as R
    from retto_amd import workload
    s = _session(lanes=1)
    try:
        # (lines of at most 10 : 1, so that every rec width stays below 648)
        planted = [workload.planted_page(320, 480, 4, seed=31, ratio_range=(3.0, 10.0)),
                   workload.planted_page(352, 640, 5, seed=32, ratio_range=(3.0, 10.0))]
        pages = [p for p, _ in planted]
        maps = [workload.planted_map(*R.resize_either_dims(*p.shape[:2]), p.shape[0], p.shape[1], rects) for p, rects in planted]
        s.profile_enable()
        off = s.run_batch(pages, det_map_override=maps)
        prof = s.profile_get()
        assert _calls(prof, "rec_window_cut") == 0 and _calls(prof, "rec_window_stitch") == 0 and _calls(prof, "net/rec") == 1
        assert sum(len(r.rec_result) for r in off) >= 2
        s.set_rec_windows(640, 128)
        s.profile_enable()
        on = s.run_batch(pages, det_map_override=maps)
        prof = s.profile_get()
        assert _calls(prof, "rec_window_cut") == 0 and _calls(prof, "rec_window_stitch") == 0 and _calls(prof, "net/rec") == 1
        for a, b in zip(on, off):
            _same(a, b)
            assert all(r.windows == 1 for r in a.rec_result) and all(r.windows == 1 for r in b.rec_result)
        # (and the labels do appear when a line is long: one of each per group)
        rpages, quads = _region_pages(40)
        s.profile_enable()
        long_one = s.run_regions(rpages[:1], quads[:1])[0]
        prof = s.profile_get()
        assert _calls(prof, "rec_window_cut") == 1 and _calls(prof, "rec_window_stitch") == 1 and _calls(prof, "net/rec") == 1
        assert [r.windows for r in long_one.rec_result] == [len(retto_amd.rec_window_plan(1300, 640, 128)["origins"])] == [3]
    finally:
        s.close()


# ---- 4. the pipeline equals the debug entry ------------------------------------------------------------------------------------
def _line_tensors(s, pages, quads, results):
    """every line's rec tensor as the pipeline made it: rt_crop_images, the classifier's rotation as the result reports it,
    rt_resize_norm_image at the batch width rec_plan gives the page's lines (one batch a page here: at most 6 lines)"""
    from oracle import ref_lib as R
    thresh = np.float32(s.config.cls_processor_config.thresh)
    out = []
    for page, q, res in zip(pages, quads, results):
        crops = s.crop_images(page, np.array(q, np.float32))
        assert len(crops) <= 6
        ratio = np.float32(320) / np.float32(48)
        for c in crops:
            ratio = max(ratio, np.float32(c.shape[1]) / np.float32(c.shape[0]))
        for c, cl in zip(crops, res.cls_result):
            if cl.label.label == 180 and np.float32(cl.label.score) >= thresh:
                c = R.rotate180(c)
            out.append(s.resize_norm_image(c, c.shape[0], c.shape[1], 48, 320, float(ratio)))
    return out


def _greedy(idx, prob):
    """pp::ctc_decode on one line's rows: the kept tokens and the mean of their probabilities, summed in f32 in row order"""
    keep = (idx != 0) & np.concatenate([[True], idx[1:] != idx[:-1]])
    acc = np.float32(0.0)
    for p in prob[keep]:
        acc = np.float32(acc + p)
    with np.errstate(invalid="ignore", divide="ignore"):
        return idx[keep], np.float32(acc / np.float32(int(keep.sum())))


def test_pipeline_equals_the_debug_entry(s32):
    pages, quads = _region_pages(60)
    s32.set_rec_windows(320, 64)
    try:
        got = s32.run_regions(pages, quads)
        lines = _line_tensors(s32, pages, quads, got)
        assert [l.shape[2] for l in lines] == [1300, 700, 480, 480]
        units, stitched, plans = s32.debug_rec_windows(lines)
    finally:
        s32.set_rec_windows(0)
    recs = [r for res in got for r in res.rec_result]
    assert [[r.windows for r in res.rec_result] for res in got] == REGION_UNITS
    assert [len(p["origins"]) for p in plans] == [n for page in REGION_UNITS for n in page]
    n_tokens = 0
    for r, (idx, prob, _z5) in zip(recs, stitched):
        tokens, score = _greedy(idx, prob)
        assert np.array_equal(r.tokens, tokens)
        assert np.float32(r.score).tobytes() == score.tobytes() or (np.isnan(score) and np.isnan(r.score))
        n_tokens += len(tokens)
    assert n_tokens > 0


# ---- 5. options ride along -------------------------------------------------------------------------------------------------------
def test_options_ride_along():
    pages, quads = _region_pages(60)
    plain = _session(lanes=1)
    try:
        plain.set_rec_windows(320, 64)
        base = plain.run_regions(pages, quads)
    finally:
        plain.close()
    cfg = retto_amd.synthetic_session_config(0, lanes=1)
    cfg.rec_processor_config.return_candidates = 2
    cfg.rec_processor_config.return_word_box = True
    s = retto_amd.RettoSession(cfg)
    try:
        s.set_rec_windows(320, 64)
        s.set_rec_beam(4, 2)
        got = s.run_regions(pages, quads)
    finally:
        s.close()
    for page, a, b in zip(pages, got, base):
        _same(a, b)
        assert [r.windows for r in a.rec_result] == [r.windows for r in b.rec_result]
        for r in a.rec_result:
            assert len(r.candidates) == len(r.tokens) == len(r.token_cols)
            assert [c[0][0] for c in r.candidates] == [int(t) for t in r.tokens]          # rank 0 of each candidate row is the token
            assert r.beams is not None and 1 <= len(r.beams) <= 2
            assert r.words is not None
            for w in r.words:
                q = np.asarray(w.box.as_array(), np.float32).reshape(-1, 2)
                assert np.isfinite(q).all()
                assert (q[:, 0] >= 0).all() and (q[:, 0] <= page.shape[1]).all() and (q[:, 1] >= 0).all() and (q[:, 1] <= page.shape[0]).all()


# ---- 6. the setter ---------------------------------------------------------------------------------------------------------------
def test_setter_is_guarded_and_a_batch_keeps_its_value():
    from oracle import ref_lib as R
    from retto_amd import workload
    s = _session(lanes=2)
    try:
        h, w = 736, 1408
        assert tuple(R.resize_either_dims(h, w)) == (h, w)
        rects = [(24, 100, 300, 130), (24, 300, 1384, 340)]
        pages = [_rand_page(h, w, 121), _rand_page(h, w, 122)]
        maps = [workload.planted_map(h, w, h, w, rects)] * 2
        for bad in ((96, 0), (130, 0), (-128, 0), (128, 48), (128, 96)):
            with pytest.raises(retto_amd.InvalidArgument):
                s.set_rec_windows(*bad)
        assert s.rec_windows == (0, 0)
        ref_off = s.run_batch(pages, det_map_override=maps)
        assert all(len(r.rec_result) == 2 and all(x.windows == 1 for x in r.rec_result) for r in ref_off)
        s.set_rec_windows(640, 128)
        ref_on = s.run_batch(pages, det_map_override=maps)
        assert all(all(x.windows > 1 for x in r.rec_result) for r in ref_on)
        s.profile_enable()
        ticket = s.submit_batch_raw(pages, [h, h], [w, w], det_map_override=maps)
        with pytest.raises(retto_amd.InvalidArgument) as e:   # refused while the ticket is in flight
            s.set_rec_windows(0)
        assert "in flight" in str(e.value)
        got = s.wait_batch(ticket)
        assert s.rec_windows == (640, 128)
        prof = s.profile_get()
        assert _calls(prof, "rec_window_cut") == 2 and _calls(prof, "rec_window_stitch") == 2   # one group on each lane
        for a, b in zip(got, ref_on):
            _same(a, b)
            assert [x.windows for x in a.rec_result] == [x.windows for x in b.rec_result]
        # the batch carries the value of its submit: changed right after the wait, the next batch runs without windows
        s.set_rec_windows(0)
        s.profile_enable()
        got_off = s.wait_batch(s.submit_batch_raw(pages, [h, h], [w, w], det_map_override=maps))
        prof = s.profile_get()
        assert _calls(prof, "rec_window_cut") == 0 and _calls(prof, "rec_window_stitch") == 0
        for a, b in zip(got_off, ref_off):
            _same(a, b)
    finally:
        s.close()

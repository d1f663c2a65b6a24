"""Sessions whose rec head is not 6625 classes wide: `classes` is whatever the model's head.fc has and the dictionary is the
caller's, yet every other GPU test of the rec network, the session and the pipeline runs synth.REC_CLASSES.  Here the synthetic
rec model's head is cut to 3, 97 and 129 classes (one 16-column group; one 128-column tile with 7 of 8 groups; a second tile
with one real column and 15 pad columns) or grown to 18385 (PP-OCRv5's count: 144 tiles), the dictionary sized to match, and the
session, the rec network, the pipeline's fused head against the un-fused rt_rec path, and the candidates of a head with fewer
classes than K are checked."""
import functools

import numpy as np
import pytest
import torch

from oracle import nets_torch as N
from oracle import ref_lib as R
from oracle.pipeline import OracleSession
import retto_amd
from retto_amd import synth, workload

pytestmark = pytest.mark.gpu

CLASS_COUNTS = (3, 97, 129, 18385)
REC_INPUT = {3: (3, 3, 48, 321), 97: (3, 3, 48, 321), 129: (3, 3, 48, 321), 18385: (2, 3, 48, 487)}


@functools.lru_cache(maxsize=None)
def models_for(classes):
    """(det, cls, rec, dictionary) blobs: the default synthetic models with rec.head.fc cut to its first `classes` columns, or
    grown past synth.REC_CLASSES by columns of the same gain (3 / sqrt(120) for the weights, 0.05 for the bias)"""
    rec = synth.rec_tensors()
    w, b = rec["rec.head.fc.w"], rec["rec.head.fc.b"]
    D, have = w.shape
    if classes > have:
        rng = np.random.default_rng(classes)
        w = np.concatenate([w, (rng.standard_normal((D, classes - have)) * 3.0 / np.sqrt(D)).astype(np.float32)], 1)
        b = np.concatenate([b, (rng.standard_normal(classes - have) * 0.05).astype(np.float32)])
    rec["rec.head.fc.w"], rec["rec.head.fc.b"] = np.ascontiguousarray(w[:, :classes]), np.ascontiguousarray(b[:classes])
    return (synth.pack_blob(synth.det_tensors()), synth.pack_blob(synth.cls_tensors()), synth.pack_blob(rec),
            synth.synth_dict(classes - 2))


def config_for(classes, dictionary=None, candidates=0, **kw):
    det, cls, rec, dic = models_for(classes)
    src = retto_amd.RettoWorkerModelSource.Blob
    cfg = retto_amd.RettoSessionConfig(**kw)
    cfg.worker_config = retto_amd.RettoHipWorkerConfig(
        device=0, models=retto_amd.RettoWorkerModelProvider(det=src(det), rec=src(rec), cls=src(cls)))
    cfg.rec_processor_config.character_source = src(dic if dictionary is None else dictionary)
    cfg.rec_processor_config.return_candidates = candidates
    return cfg


@pytest.fixture(scope="module")
def sessions():
    """session(classes, **config): created on first use, once per module"""
    made = {}

    def get(classes, **kw):
        key = (classes, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = retto_amd.RettoSession(config_for(classes, **kw))
        return made[key]
    yield get
    for s in made.values():
        s.close()


@functools.lru_cache(maxsize=None)
def oracle_for(classes):
    return OracleSession(*models_for(classes))


@functools.lru_cache(maxsize=None)
def planted():
    h, w = 480, 704
    page, rects = workload.planted_page(h, w, 5, 21)
    dh, dw = R.resize_either_dims(h, w)
    return page, workload.planted_map(dh, dw, h, w, rects)


@pytest.mark.parametrize("classes", CLASS_COUNTS)
def test_session_reports_its_class_count(sessions, classes):
    s = sessions(classes)
    assert s._hd.lib.rt_rec_classes(s._hd.h) == classes
    assert len(oracle_for(classes).dict) == classes


def test_dictionary_of_another_size_is_refused():
    with pytest.raises(retto_amd.ShapeError) as e:
        retto_amd.RettoSession(config_for(97, dictionary=synth.synth_dict()))
    assert "6625" in str(e.value) and "97" in str(e.value)


@pytest.mark.parametrize("classes", CLASS_COUNTS)
def test_rec_net(sessions, classes):
    """test_gpu_parity.test_rec_net at this class count: rt_rec against the torch oracle"""
    shape = REC_INPUT[classes]
    x = np.random.default_rng(shape[3]).uniform(-1, 1, shape).astype(np.float32)
    x[:, :, :, shape[3] // 2:] = 0.0
    got = sessions(classes).worker.rec(x)
    ref = N.rec_forward(oracle_for(classes).wr, torch.from_numpy(x)).numpy()
    assert got.shape == ref.shape and got.shape[0] == shape[0] and got.shape[2] == classes
    err = np.abs(got - ref).max()
    top2 = np.sort(ref, -1)[..., -2:]
    decisive = (top2[..., 1] - top2[..., 0]) > 1e-4
    print("classes %d: max abs err %.3g, decisive share %.3f" % (classes, err, decisive.mean()))
    assert err <= 2e-4
    assert (got.argmax(-1)[decisive] == ref.argmax(-1)[decisive]).all()
    assert decisive.mean() >= 0.95


def _teacher_forced(s, classes):
    """test_gpu_parity.test_pipeline_teacher_forced on one planted page: the pipeline (fused head) against the oracle pipeline
    fed by the same session's workers (rt_rec: logits, softmax, argmax as separate launches)"""
    page, pmap = planted()
    r = s.run_batch([page], det_map_override=[pmap])[0]
    det, cls, rec, dic = models_for(classes)
    o = OracleSession(det, cls, rec, dic)
    o.det_worker, o.cls_worker, o.rec_worker = s.worker.det, s.worker.cls, s.worker.rec
    ref = o.run(page, det_map_override=pmap)
    assert len(r.det_result) == len(ref.det_boxes) == 5
    assert np.array_equal(np.stack([d.boxes.as_array() for d in r.det_result]), ref.det_boxes)
    assert [c.label.label for c in r.cls_result] == list(ref.cls_labels)
    assert sum(len(t) for t in ref.rec_tokens) > 0
    for k, (g, t) in enumerate(zip(r.rec_result, ref.rec_tokens)):
        assert np.array_equal(g.tokens, t), "line %d tokens differ" % k
        assert g.text == ref.rec_text[k]
    np.testing.assert_allclose([g.score for g in r.rec_result], ref.rec_scores, rtol=1e-4, equal_nan=True)
    return r


@pytest.mark.parametrize("classes", CLASS_COUNTS)
def test_pipeline_teacher_forced(sessions, classes):
    _teacher_forced(sessions(classes), classes)


def test_pipeline_teacher_forced_f16(sessions):
    """the fp16 networks end in the same fp32 head"""
    _teacher_forced(sessions(97, dtype="f16"), 97)


def test_candidates_of_a_three_class_head(sessions):
    """K = 5 over 3 classes: ranks 0 .. 2 are the three classes, the token first and the others by probability, ranks 3 and 4
    are (-1, 0.0); the three probabilities are a whole softmax row, so they sum to 1"""
    r = _teacher_forced(sessions(3, candidates=5), 3)
    tokens = 0
    for g in r.rec_result:
        assert len(g.candidates) == len(g.tokens)
        for t, cand in zip(g.tokens, g.candidates):
            assert len(cand) == 5
            assert cand[0][0] == int(t)
            assert sorted(c[0] for c in cand[:3]) == [0, 1, 2]
            assert cand[1][2] >= cand[2][2] >= 0.0
            assert all((c[0], c[2]) == (-1, 0.0) for c in cand[3:])
            assert abs(sum(float(c[2]) for c in cand[:3]) - 1.0) <= 1e-5
            tokens += 1
    assert tokens > 0

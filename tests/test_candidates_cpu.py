"""Token candidates (rt_config.rec_return_candidates) without a GPU: the config plumbing, and rt_debug_ctc_candidates_host --
retto_amd/csrc/ctc_candidates.h in plain fp32 loops on the CPU -- against the fp64 restatement in ctc_candidates_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_candidates_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fp32 logits of 120 products of magnitude up to ~2.6 each carry an accumulated rounding error of order 1e-5; a softmax
# probability moves by at most p (1 - p) <= 1/4 of a logit error, plus a few ulp of expf and of the 6625-term sum.  An fp32
# emulation of the rule on 240 rows of the synthetic rec net measured a worst |p - q| of 5.0e-6 against fp64 (it fails at 2e-6
# and passes at 2e-5); 4 x that is the tolerance.
TOL = 2e-5


def run_host(z, W, b, idx, prob, tpl, K):
    lib = _lib.load()
    rows = int(sum(tpl))
    cands, cols = R.new_outputs(rows, K)
    ntok = np.full(len(tpl), -1, np.int32)
    keep, a = R.call_args(z, W, b, idx, prob, tpl)
    rc = lib.rt_debug_ctc_candidates_host(a[0], a[1], a[2], W.shape[1], a[3], a[4], a[5], len(tpl), K,
                                          cands.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p),
                                          ntok.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return cands, cols, ntok


def test_config_defaults_off():
    c = _lib.Config(); _lib.load().rt_config_default(C.byref(c))
    assert c.rec_return_candidates == 0 and c.struct_size == C.sizeof(_lib.Config)
    assert retto_amd.RecProcessorConfig().return_candidates == 0
    r = retto_amd.RecProcessorSingleResult("", 0.0)
    assert r.candidates is None and r.token_cols is None
    assert _lib.MAX_CANDIDATES == 8
    assert "#define RT_MAX_CANDIDATES 8" in open(os.path.join(ROOT, "include", "retto_hip.h")).read()


@pytest.mark.parametrize("bad", [-1, 9])
def test_rt_create_rejects_values_outside_0_to_8(bad):
    """checked before any device is touched"""
    lib = _lib.load()
    lib.rt_last_error.restype = C.c_char_p
    c = _lib.Config(); lib.rt_config_default(C.byref(c))
    c.rec_return_candidates = bad
    h = C.c_void_p()
    assert lib.rt_create(C.byref(c), C.byref(h)) == retto_amd.InvalidArgument.code and not h.value
    assert b"rec_return_candidates" in lib.rt_last_error(None)


@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("N", [5, 37, 64, 65, 6625])
def test_host_rule_against_fp64(N, K):
    rng = np.random.default_rng(1000 * N + K)
    tpl = [40, 1, 25, 7] if N == 6625 else [40, 1, 80, 7, 33]
    z, W, b, idx, prob = R.make_case(rng, N, tpl)
    cands, cols, ntok = run_host(z, W, b, idx, prob, tpl, K)
    assert 0 < ntok.sum() < sum(tpl)
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, tpl, K, TOL, (N, K))


def test_fill_when_fewer_classes_than_candidates():
    rng = np.random.default_rng(5)
    tpl = [30]
    z, W, b, idx, prob = R.make_case(rng, 5, tpl)
    cands, cols, ntok = run_host(z, W, b, idx, prob, tpl, 8)
    assert ntok[0] > 0
    for j in range(ntok[0]):
        ids = cands["id"][j]
        assert sorted(ids[:5]) == [0, 1, 2, 3, 4]   # the token and the four other classes, the blank among them
        assert list(ids[5:]) == [-1, -1, -1] and np.all(cands["prob"][j][5:] == 0.0)
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, tpl, 8, TOL)


def test_exact_ties_are_ordered_by_id():
    """All-zero features: every logit is exactly its bias, and classes with the same bias come out in id order."""
    N, K, T = 37, 8, 6
    b = np.array([0.5, 2.0, 1.0] * 12 + [2.0], np.float32)   # ids 1, 4, 7, ... and 36 share the top value
    z = np.zeros((T, R.D), np.float32)
    W = np.random.default_rng(3).normal(0, 1, (R.D, N)).astype(np.float32)
    idx = np.array([4, 0, 1, 1, 36, 2], np.int32)
    prob = np.full(T, 0.25, np.float32)
    cands, cols, ntok = run_host(z, W, b, idx, prob, [T], K)
    assert ntok[0] == 4 and list(cols[:4]) == [0, 2, 4, 5]
    top = [i for i in range(N) if b[i] == 2.0]
    for j, tok in enumerate([4, 1, 36, 2]):
        want = [i for i in top if i != tok][:K - 1]
        assert list(cands["id"][j][1:]) == want, (j, cands["id"][j])
        assert len(set(cands["prob"][j][1:].tobytes()[4 * k:4 * k + 4] for k in range(K - 1))) == 1   # bit-equal
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, [T], K, TOL)


@pytest.mark.parametrize("K", [1, 3])
def test_kept_rule_cases(K):
    """An all-blank line, repeats, T = 1 (kept and blank), an empty line followed by a non-empty one."""
    N = 37
    lines = [[0, 0, 0, 0], [5, 5, 0, 5, 5, 7, 7, 7, 0, 0, 9], [3], [0], [], [2, 2, 6], []]
    tpl = [len(l) for l in lines]
    idx = np.array([v for l in lines for v in l], np.int32)
    rng = np.random.default_rng(9)
    z = rng.normal(0, 5, (len(idx), R.D)).astype(np.float32)
    W = (rng.normal(0, 1, (R.D, N)) * np.sqrt(2.0 / R.D)).astype(np.float32)
    b = rng.normal(0, 0.5, N).astype(np.float32)
    prob = rng.random(len(idx)).astype(np.float32)
    cands, cols, ntok = run_host(z, W, b, idx, prob, tpl, K)
    assert list(ntok) == [0, 4, 1, 0, 0, 2, 0]
    assert list(cols[4:8]) == [0, 3, 5, 10] and list(cols[15:16]) == [0] and list(cols[17:19]) == [0, 2]
    R.check_outputs(cands, cols, ntok, z, W, b, idx, prob, tpl, K, TOL)


def test_k1_needs_no_features():
    idx = np.array([3, 3, 4], np.int32); prob = np.array([0.5, 0.6, 0.7], np.float32)
    lib = _lib.load()
    cands, cols = R.new_outputs(3, 1); ntok = np.zeros(1, np.int32)
    tpl = np.array([3], np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rt_debug_ctc_candidates_host(None, None, None, 10, P(idx), P(prob), P(tpl), 1, 1, P(cands), P(cols), P(ntok)) == 0
    assert ntok[0] == 2 and list(cols[:2]) == [0, 2] and list(cands["id"][:2, 0]) == [3, 4]
    assert list(cands["prob"][:2, 0]) == [np.float32(0.5), np.float32(0.7)]
    # bad arguments: K out of range, features missing at K > 1, an argmax outside the classes
    assert lib.rt_debug_ctc_candidates_host(None, None, None, 10, P(idx), P(prob), P(tpl), 1, 9, P(cands), P(cols), P(ntok)) == 8
    assert lib.rt_debug_ctc_candidates_host(None, None, None, 10, P(idx), P(prob), P(tpl), 1, 2, P(cands), P(cols), P(ntok)) == 8
    assert lib.rt_debug_ctc_candidates_host(None, None, None, 4, P(idx), P(prob), P(tpl), 1, 1, P(cands), P(cols), P(ntok)) == 8
    # the device form rejects a null session before any device work
    assert lib.rt_debug_ctc_candidates(None, None, None, None, 10, P(idx), P(prob), P(tpl), 1, 1, 0, P(cands), P(cols), P(ntok)) == 8


def test_python_mapping():
    """rt_candidate rows -> RecProcessorSingleResult.candidates entries (id, text, prob)."""
    entries = ["blank", "a", "b", " "]
    arr = (_lib.Candidate * 6)()
    for k, (i, p) in enumerate([(1, 0.75), (2, 0.125), (-1, 0.0), (3, 0.5), (0, 0.25), (1, 0.125)]):
        arr[k].id, arr[k].prob = i, p
    out = retto_amd._candidate_lists(arr, 3, 2, entries)
    assert out == [[(1, "a", 0.75), (2, "b", 0.125), (-1, "", 0.0)], [(3, " ", 0.5), (0, "blank", 0.25), (1, "a", 0.125)]]
    assert C.sizeof(_lib.Candidate) == 8 and R.CAND.itemsize == 8


def test_handle_passes_the_option_through(monkeypatch):
    """RecProcessorConfig.return_candidates reaches rt_config.rec_return_candidates (rt_create stubbed: no device here)."""
    seen = {}
    lib = _lib.load()

    class Stub:
        def __getattr__(self, name):
            return getattr(lib, name)

        def rt_create(self, cfg, out):
            seen["k"] = cfg._obj.rec_return_candidates
            return 0

        def rt_destroy(self, h):
            return None
    monkeypatch.setattr(_lib, "load", lambda: Stub())
    cfg = retto_amd.synthetic_session_config(0)
    cfg.rec_processor_config.return_candidates = 5
    retto_amd._Handle(cfg)
    assert seen["k"] == 5


def test_cli_flag():
    from retto_amd import cli
    assert cli.build_parser().parse_args(["-i", "x"]).rec_candidates == 0
    assert cli.build_parser().parse_args(["-i", "x", "--rec-candidates", "5"]).rec_candidates == 5

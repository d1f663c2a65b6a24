"""Rec lexicons (retto_amd/csrc/ctc_lexicon.h) on the MI355X: the device path (the row gather in chunks of whole lines, the CTC FC
GEMM, k_ctc_row_lse, k_ctc_lexicon_forward, k_ctc_lexicon_topk) through rt_debug_ctc_lexicon against the fp64 restatement in
ctc_lexicon_ref.py.  The checks are margin-free and leave no line and no entry out (ctc_lexicon_ref.check_outputs).

Measured on an MI355X over the grid of test_device_rule_against_fp64 (N in 5, 65, 6625; per N five lexicons of 1, 3, 4, 5 and 257
entries whose lengths are exactly 1, 7, 8, 15, 16, 31; 25 lines of 1 .. 40 steps; fp64 reference on the same features):
worst |loglik - fp64| = 1.851e-4 (N = 65; 9.75e-5 at N = 5, 1.73e-4 at N = 6625), worst |posterior - fp64| = 1.185e-5 (N = 6625).
ctc_lexicon_ref.HOOK_TOL / HOOK_PTOL are four times the one and the other.  On the grid's inputs the fp64 gap between a line's two best entries is
at least ten times HOOK_TOL (test_lexicon_cpu.test_grid_inputs_leave_a_margin_on_every_line), so rank 0 is the fp64 winner itself,
which test_device_rule_against_fp64 asserts as well."""
import numpy as np
import pytest

from retto_amd import _lib

import ctc_lexicon_ref as LR

pytestmark = pytest.mark.gpu

TOL, PTOL = LR.HOOK_TOL, LR.HOOK_PTOL


def run_dev(sess, case, chunk=0, want_table=True):
    lib = _lib.load()
    rc, out = LR.call(lib.rt_debug_ctc_lexicon, sess._hd.h, *case, chunk=chunk, want_table=want_table)
    assert rc == 0, lib.rt_last_error(sess._hd.h)
    return out


def run_host(case):
    rc, out = LR.call(_lib.load().rt_debug_ctc_lexicon_host, None, *case)
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def grid():
    """the grid's inputs and their fp64 reference, computed once"""
    out = {}
    for N in LR.GRID_N:
        case = LR.grid_case(N)
        out[N] = (case, LR.reference(*case))
    return out


@pytest.mark.parametrize("N", LR.GRID_N)
def test_device_rule_against_fp64(hip_session, grid, N):
    case, ref = grid[N]
    z, W, b, tpl, line_lex, lexicons = case
    out = run_dev(hip_session, case)
    print("N=%d:" % N, end=" ")
    wl, wp = 0.0, 0.0
    rows = LR.split_table(out["table"], line_lex, lexicons)
    for i, r in enumerate(ref):   # (the figures first: they are printed even when the check below fails)
        f = np.isfinite(r[0]) & np.isfinite(rows[i])
        if f.any():
            wl = max(wl, float(np.abs(rows[i][f] - r[0][f]).max()))
        for j in range(max(int(out["n"][i]), 0)):
            e = int(out["matches"][i]["entry"][j])
            if 0 <= e < len(r[1]):
                wp = max(wp, abs(float(out["matches"][i]["posterior"][j]) - r[1][e]))
    print("worst |loglik - fp64| %.3e, worst |posterior - fp64| %.3e" % (wl, wp))
    LR.check_outputs(out, ref, tpl, line_lex, lexicons, TOL, PTOL, N)
    assert out["n"].max() == LR.MATCHES and out["n"].min() == 0
    for i, (ll, _) in enumerate(ref):   # rank 0 is the fp64 winner (the inputs leave a margin on every line)
        if out["n"][i] > 0:
            assert out["matches"][i]["entry"][0] == int(np.argmax(ll)), (N, i)


@pytest.mark.parametrize("N", LR.GRID_N)
def test_host_and_device_tables_agree(hip_session, grid, N):
    case, ref = grid[N]
    z, W, b, tpl, line_lex, lexicons = case
    if N == 6625:   # (the host's plain loops: the three small lexicons' lines)
        keep = [i for i, k in enumerate(line_lex) if k <= 3]
        offs = np.concatenate([[0], np.cumsum(tpl)])
        z = np.concatenate([z[offs[i]:offs[i + 1]] for i in keep])
        tpl = [tpl[i] for i in keep]; line_lex = [line_lex[i] for i in keep]
        case = (z, W, b, tpl, line_lex, lexicons)
    dev, host = run_dev(hip_session, case), run_host(case)
    assert np.array_equal(np.isneginf(dev["table"]), np.isneginf(host["table"]))
    f = np.isfinite(host["table"])
    assert np.abs(dev["table"][f].astype(np.float64) - host["table"][f]).max() <= 2 * TOL   # (each within TOL of fp64)
    assert np.array_equal(dev["n"], host["n"])
    for i in range(len(tpl)):
        n = dev["n"][i]
        assert np.array_equal(dev["matches"][i]["entry"][:n], host["matches"][i]["entry"][:n]), i   # (the margin again)
        assert np.abs(dev["matches"][i]["posterior"][:n].astype(np.float64) - host["matches"][i]["posterior"][:n]).max(initial=0) <= 2 * PTOL


def test_duplicate_entries_tie_and_come_out_by_index(hip_session):
    """all-zero features: the logits are the biases, bit for bit, so equal entries have bit-equal likelihoods"""
    N, T = 6625, 6
    bias = np.random.default_rng(3).normal(-6.0, 0.3, N).astype(np.float32)
    bias[[7, 4000]] = 4.0; bias[0] = 3.0
    z, W, b = LR.zero_feature_case(N, bias, T)
    lex = [[9], [7, 4000], [7], [5, 5], [7], [7, 4000], [6624, 1, 2, 3, 4, 5, 6], [7], [7], [7, 4000]] + [[7]] * 70
    case = (z, W, b, [T], [1], [lex])
    out = run_dev(hip_session, case)
    LR.check_outputs(out, LR.reference(*case), [T], [1], [lex], TOL, PTOL)
    m = out["matches"][0]
    assert out["n"][0] == 4 and m["entry"].tolist() == [1, 5, 9, 2]
    assert m["loglik"][0].tobytes() == m["loglik"][1].tobytes() == m["loglik"][2].tobytes()
    assert m["posterior"][0].tobytes() == m["posterior"][1].tobytes() == m["posterior"][2].tobytes()
    table = out["table"][:len(lex)]
    assert np.isneginf(table[6]) and len({table[i].tobytes() for i in [2, 4, 7, 8] + list(range(10, 80))}) == 1
    assert np.array_equal(run_host(case)["matches"]["entry"], out["matches"]["entry"])


@pytest.mark.parametrize("N", [5, 65, 6625])
def test_pad_columns_take_no_part(hip_session, N):
    """negative biases: a pad column of the logits GEMM (weights and bias zero: logit 0) would raise every lse"""
    rng = np.random.default_rng(N)
    bias = (-1.0 - 3.0 * rng.random(N)).astype(np.float32)
    T = 9
    z, W, b = LR.zero_feature_case(N, bias, T)
    lex = [[N - 1], [N - 1, N - 2], [1, 1, N - 3], [2], [N - 1, 1, N - 1, 1, N - 1, 1, N - 1, 1, N - 1]]
    case = (z, W, b, [T], [1], [lex])
    ref = LR.reference(*case)
    out = run_dev(hip_session, case)
    LR.check_outputs(out, ref, [T], [1], [lex], TOL, PTOL, N)
    # what counting the pad columns would cost: log(1 + (-N % 4) / sum exp(bias)) per step, far above the tolerance
    assert T * np.log1p((-N % 4) / np.exp(bias.astype(np.float64)).sum()) > 10 * TOL
    assert np.isfinite(out["table"][:5]).all()


def test_chunks_of_whole_lines(hip_session):
    """chunk_rows = 16 with lines of 7, 9 and 20 steps: 7 + 9 fill a chunk exactly, 20 is longer than the chunk, 9 + 7 + 1 would
    pass its edge by one row; the results do not depend on the chunking"""
    rng = np.random.default_rng(16)
    N = 65
    tpl = [7, 9, 20, 9, 7, 1, 7, 20, 9, 0, 7]
    line_lex = [1, 2, 1, 2, 0, 1, 1, 2, 1, 2, 2]
    W = (rng.normal(0.0, 1.0, (LR.D, N)) * np.sqrt(2.0 / LR.D)).astype(np.float32)
    b = rng.normal(0.0, 0.5, N).astype(np.float32)
    lexicons = [[LR.random_entry(rng, N, L, 20) for L in (1, 3, 7, 8, 2, 5, 15)], [LR.random_entry(rng, N, L, 9) for L in (4, 1, 7, 2, 8)]]
    paths = [(T, None if k == 0 or T < LR.need(lexicons[k - 1][2]) else LR.alignment(lexicons[k - 1][2], T)) for T, k in zip(tpl, line_lex)]
    z = LR.planted_features(rng, W.astype(np.float64), paths)
    case = (z, W, b, tpl, line_lex, lexicons)
    ref = LR.reference(*case)
    out = run_dev(hip_session, case, chunk=16)
    LR.check_outputs(out, ref, tpl, line_lex, lexicons, TOL, PTOL)
    assert out["n"][9] == 0 and out["n"][4] == 0
    whole = run_dev(hip_session, case)
    assert np.array_equal(np.isneginf(whole["table"]), np.isneginf(out["table"]))
    LR.check_outputs(whole, ref, tpl, line_lex, lexicons, TOL, PTOL)
    for c in (1, 7, 36):
        LR.check_outputs(run_dev(hip_session, case, chunk=c), ref, tpl, line_lex, lexicons, TOL, PTOL, c)


def test_mixed_lexicon_ids_and_untouched_lines(hip_session, grid):
    """line_lex mixing 0, lexicon 1 and lexicon 2 in one call: a line of lexicon 0 gets 0 matches, owns no slot of the table, and
    its match slots keep the canary (check_outputs); the other lines' results are those of a call of their own"""
    case, _ = grid[65]
    z, W, b, tpl, line_lex, lexicons = case
    two = [lexicons[4], lexicons[1]]
    mixed = [0, 1, 2, 0, 2, 1, 0, 0, 1, 2] + [0] * (len(tpl) - 10)
    mcase = (z, W, b, tpl, mixed, two)
    ref = LR.reference(*mcase)
    out = run_dev(hip_session, mcase)
    LR.check_outputs(out, ref, tpl, mixed, two, TOL, PTOL)
    assert len(out["table"]) == sum(len(two[k - 1]) for k in mixed if k) and not (out["table"] == LR.CANARY_F).any()
    assert (out["n"][[i for i, k in enumerate(mixed) if k == 0]] == 0).all()
    # a line's values do not depend on what else is in the call: line 5 (lexicon 1) alone
    offs = np.concatenate([[0], np.cumsum(tpl)])
    alone = run_dev(hip_session, (z[offs[5]:offs[6]], W, b, [tpl[5]], [1], two))
    assert alone["matches"][0]["entry"].tolist() == out["matches"][5]["entry"].tolist()
    # without the table the matches are the same, and no line at all is no work at all
    assert run_dev(hip_session, mcase, want_table=False)["matches"].tobytes() == out["matches"].tobytes()
    none = run_dev(hip_session, (z, W, b, tpl, [0] * len(tpl), two))
    assert (none["n"] == 0).all() and (none["matches"]["entry"] == LR.CANARY_ENTRY).all()


def test_bad_arguments_are_rejected(hip_session):
    lib = _lib.load()
    z, W, b = LR.zero_feature_case(5, [-1.0] * 5, 4)
    f, h = lib.rt_debug_ctc_lexicon, hip_session._hd.h
    for case, chunk, msg in ((([4], [2], [[[1]]]), 0, b"line 0 names lexicon 2, outside [0, 1]"),
                             (([4], [1], [[[5]]]), 0, b"class id 5 in entry 0 is outside [1, 5)"),
                             (([4], [1], [[[1] * 32]]), 0, b"entry 0 has 32 ids"),
                             (([-4], [1], [[[1]]]), 0, b"line 0 has a negative number of time steps"),
                             (([4], [1], [[[1]]]), -1, b"chunk_rows is negative")):
        assert LR.call(f, h, z, W, b, *case, chunk=chunk)[0] == 8
        assert msg in lib.rt_last_error(h), lib.rt_last_error(h)   # each failure has its own message

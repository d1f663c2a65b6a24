"""The rec language model (retto_amd/csrc/ctc_lm.h) without a GPU: the ARPA parser and compiler (rt_debug_lm_compile) round the
writer of ctc_lm_ref.py, with <sp>, <unk>, <s>, the dropped n-grams and every refusal with its message; the compiled automaton
walked on the host (rt_debug_lm_score) against the model's direct fp64 definition; and the surface: exports, header, Python
mirror."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_lm_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT_BYTES = "a\nb\nc\nd\né\n".encode("utf-8")
DICT = ["blank", "a", "b", "c", "d", "é", " "]     # what the library reads DICT_BYTES as: the blank first, the space last
CLASSES = len(DICT)


def compile_ok(arpa, **kw):
    rc, got, msg = MR.compile_call(_lib.load(), DICT_BYTES, arpa, **kw)
    assert rc == 0, msg
    assert got["classes"] == CLASSES
    return got


def small_model(order=3, seed=1):
    # texts with the space (class 6) and the two-byte entry (class 5), so that both are tokens of higher orders
    return MR.random_model(seed, CLASSES, order, texts=[(1, 6, 5, 2, 1), (6, 6, 1), (5, 5, 6, 2)])


# ---------------------------------------------------------------- parser
@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_parser_round_trip_through_the_writer(order):
    m = small_model(order)
    assert m.order == order
    got = compile_ok(MR.write_arpa(m, DICT), oov_log10=-6.5)
    ids, lens, logp, bo = m.id_form()
    assert got["ids"].tolist() == ids.tolist() and got["lens"].tolist() == lens.tolist()
    assert got["logp"].tobytes() == logp.tobytes() and got["backoff"].tobytes() == bo.tobytes()
    assert (got["order"], got["dropped"], got["states"]) == (order, 0, len(m.state_index))
    assert got["oov"] == np.float32(np.float64(np.float32(-6.5)) * MR.LN10)


def test_parser_sp_unk_and_s():
    m = small_model(3)
    text = MR.write_arpa(m, DICT, unk=-5.5)
    assert "<sp>" in text and "<s>" in text and "\t<unk>" in text and " \t" not in text
    got = compile_ok(text, oov_log10=-1.0)
    assert got["oov"] == np.float32(-5.5 * MR.LN10)                   # <unk>'s unigram wins over the caller's value
    assert got["lens"].tolist() == m.id_form()[1].tolist()            # ... and is not an n-gram of the id form
    grams, o = [], 0
    for L in got["lens"]:
        grams.append(tuple(got["ids"][o:o + L])); o += L
    assert (CLASSES,) in grams and any(g[0] == CLASSES and len(g) > 1 for g in grams)   # <s> is the pseudo-class `classes`
    assert all(CLASSES not in g[1:] and 0 not in g for g in grams)
    assert any(6 in g for g in grams) and any(5 in g for g in grams)
    # spaces in place of tabs, CRLF line ends and a preamble read the same
    loose = "a preamble line\r\n" + text.replace("\t", "  ").replace("\n", "\r\n")
    again = compile_ok(loose, oov_log10=-1.0)
    assert all(np.array_equal(got[k], again[k]) for k in ("ids", "lens", "logp", "backoff"))


def test_parser_drops_and_counts():
    m = small_model(3)
    extra = ((1, "-1.0\tzz"), (1, "-1.0\t</s>"), (2, "-1.0\ta </s>"), (2, "-1.0\ta <s>"), (2, "-1.0\t<unk> a"), (2, "-0.5\tzz a\t-0.1"),
             (3, "-1.0\ta zz a"))
    got = compile_ok(MR.write_arpa(m, DICT, extra=extra))
    assert got["dropped"] == len(extra)
    assert got["lens"].tolist() == m.id_form()[1].tolist() and got["logp"].tobytes() == m.id_form()[2].tobytes()


def arpa_lines(uni=(), bi=(), tri=(), head=None, end=True):
    out = ["\\data\\"] + (head if head is not None else ["ngram 1=%d" % len(uni), "ngram 2=%d" % len(bi), "ngram 3=%d" % len(tri)])
    for k, sec in ((1, uni), (2, bi), (3, tri)):
        out += ["", "\\%d-grams:" % k] + list(sec)
    return "\n".join(out + (["", "\\end\\"] if end else [])) + "\n"


REFUSALS = [
    ("nan", arpa_lines(uni=["nan\ta"]), "line 7: a number is not finite"),
    ("inf", arpa_lines(uni=["-1\ta\t-inf"]), "line 7: a number is not finite"),
    ("overflow", arpa_lines(uni=["-1e999\ta"]), "line 7: a number is not finite"),
    ("beyond float32", arpa_lines(uni=["-2e38\ta"]), "line 7: a number is not finite"),
    ("not a number", arpa_lines(uni=["-1x\ta"]), "line 7: a number does not parse"),
    ("duplicate", arpa_lines(uni=["-1\ta", "-1\tb", "-2\ta"]), "line 9: the n-gram is there twice"),
    ("context", arpa_lines(uni=["-1\ta"], bi=["-1\tb a"]), "line 10: the n-gram's context (its first 1 tokens) is not an n-gram"),
    ("context of a trigram", arpa_lines(uni=["-1\ta"], bi=["-1\ta a"], tri=["-1\ta a a", "-1\ta b a"]),
     "line 14: the n-gram's context (its first 2 tokens) is not an n-gram"),
    ("order in data", arpa_lines(head=["ngram 1=0", "ngram 6=1"]), "line 3: order 6 is above RT_MAX_LM_ORDER (5)"),
    ("order of a section", "\\data\\\nngram 1=1\n\n\\6-grams:\n\\end\\\n", "line 4: order 6 is above RT_MAX_LM_ORDER (5)"),
    ("undeclared section", "\\data\\\nngram 1=1\n\n\\2-grams:\n\\end\\\n", "line 4: a section of order 2 that \\data\\ does not declare"),
    ("fields", arpa_lines(uni=["-1\ta\t-1\t-1"]), "line 7: a 1-gram line needs 2 or 3 fields, not 4"),
    ("count line", arpa_lines(head=["ngrams 1=1"]), "line 2: not an \"ngram k=count\" line"),
    ("truncated", arpa_lines(uni=["-1\ta"], end=False), "the file ends without \\end\\"),
    ("no data", "hello\n", "no \\data\\ section"),
    ("unk above 0", arpa_lines(uni=["0.5\t<unk>"]), "line 7: <unk>'s log-probability is above 0"),
]


@pytest.mark.parametrize("name,text,want", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_parser_refusals_name_the_line(name, text, want):
    rc, got, msg = MR.compile_call(_lib.load(), DICT_BYTES, text)
    assert rc == 8 and want in msg and msg.startswith("lm: line "), (rc, msg)
    assert len(got["lens"]) == 0 and got["states"] == 0


def test_compile_hook_arguments():
    lib = _lib.load()
    text = MR.write_arpa(small_model(3), DICT)
    for oov in (0.5, float("nan"), float("-inf")):
        rc, _got, msg = MR.compile_call(lib, DICT_BYTES, text, oov_log10=oov)
        assert rc == 8 and "oov_log10 is not a finite number at most 0" in msg
    rc, got, msg = MR.compile_call(lib, DICT_BYTES, text, cap=3)     # a cap too small: the counts still come back
    assert rc == 8 and "the model needs 165 ids and 65 n-grams" in msg and (got["lens"] == 0).all() and (got["ids"] == 0).all()
    assert (got["order"], got["states"]) == (3, len(small_model(3).state_index))
    err = C.create_string_buffer(64)
    assert lib.rt_debug_lm_compile(DICT_BYTES, len(DICT_BYTES), None, 5, 0.0, None, 0, None, None, None, 0, None, None, None, None, None,
                                   None, None, err, 64) == 8 and b"bad argument" in err.value
    rc, _got, msg = MR.compile_call(lib, b"\xff\n", text)
    assert rc == 5 and "UTF-8" in msg


# ---------------------------------------------------------------- the id form
def test_id_form_refusals_name_the_n_gram():
    lib = _lib.load()
    m = MR.Model(5, {(1,): (-1.0, -0.5), (2,): (-1.0, -0.5), (1, 2): (-0.5, 0.0)}, -9.0)
    f32, i32 = np.float32, np.int32
    base = m.id_form()

    def with_(ids=None, lens=None, logp=None, bo=None):
        return (np.array(base[0] if ids is None else ids, i32), np.array(base[1] if lens is None else lens, i32),
                np.array(base[2] if logp is None else logp, f32), np.array(base[3] if bo is None else bo, f32))

    cases = [(with_(ids=[1, 0, 1, 2]), {}, "n-gram 1: the blank (class 0) is not a token"),
             (with_(ids=[1, 2, 1, 6]), {}, "n-gram 2: token id 6 is outside [1, 5]"),
             (with_(ids=[1, 2, 1, 5]), {}, "n-gram 2: token id 5 (<s>) past the first place"),
             (with_(ids=[1, 1, 1, 2]), {}, "n-gram 1: the n-gram is there twice"),
             (with_(ids=[1, 2, 3, 2]), {}, "n-gram 2: the n-gram's context (its first 1 tokens) is not an n-gram"),
             (with_(logp=[-1.0, np.nan, -0.5]), {}, "n-gram 1: a number is not finite"),
             (with_(bo=[-np.inf, -0.5, 0.0]), {}, "n-gram 0: a number is not finite"),
             (with_(lens=[1, 1, 6]), {}, "n-gram 2: an n-gram of 6 tokens, outside [1, RT_MAX_LM_ORDER (5)]"),
             (with_(lens=[1, 0, 2]), {}, "n-gram 1: an n-gram of 0 tokens"),
             (base, {"oov": 0.5}, "oov is not a finite number at most 0"), (base, {"oov": float("nan")}, "oov is not a finite number"),
             (base, {"classes": 1}, "at least 2 classes")]
    for form, kw, want in cases:
        rc, lm, st, msg = MR.score_call(lib, m, [(1, 2)], id_form=form, **kw)
        assert rc == 8 and want in msg and msg.startswith("rt_debug_lm_score: lm: "), (want, msg)
        assert lm[0] == MR.CANARY_LM
    # the count limit, without reading the n-grams' ids
    n = MR.MAX_NGRAMS + 1
    big = (np.ones(8, i32), np.ones(n, i32), np.zeros(n, f32), np.zeros(n, f32))
    rc, _lm, _st, msg = MR.score_call(lib, m, [(1,)], id_form=big)
    assert rc == 8 and "4194305 n-grams, outside [0, RT_MAX_LM_NGRAMS (4194304)]" in msg
    # a string with the blank, <s> or a foreign class is refused too
    for s in ((0,), (5,), (1, 7)):
        rc, _lm, _st, msg = MR.score_call(lib, m, [s])
        assert rc == 8 and "is outside [1, 5)" in msg
    rc, lm, st, _msg = MR.score_call(lib, m, [])
    assert rc == 0 and lm[0] == MR.CANARY_LM


# ---------------------------------------------------------------- the automaton
@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_automaton_is_the_direct_definition(order):
    """random strings with OOV classes and contexts deeper than the order, and every n-gram of the model itself as a string:
    lm within float32 rounding of the fp64 definition (at most 13 tokens of at most 5 additions each and 13 more for the sum,
    each off by at most 2^-24 of a running sum no larger than the result: 78 * 6e-8 = 4.7e-6, held to 1e-5), the final state the
    longest suffix of <s> + string that is a state"""
    N = 12
    rng = np.random.default_rng(50 + order)
    texts = [tuple(int(c) for c in rng.integers(1, N, 9)) for _ in range(6)]
    m = MR.random_model(70 + order, N, order, texts, per_level=60)
    assert m.order == order
    unigrams = {g[0] for g in m.grams if len(g) == 1}
    assert any(c not in unigrams for c in range(1, N))
    strings = [()] + texts + [t[:k] for t in texts for k in range(1, 9)]
    strings += [tuple(int(c) for c in rng.integers(1, N, int(rng.integers(1, 14)))) for _ in range(300)]
    strings += [g[1:] if g[0] == N else g for g in m.grams]
    rc, lm, st, msg = MR.score_call(_lib.load(), m, strings)
    assert rc == 0, msg
    depth = set()
    for s, v, q in zip(strings, lm, st):
        want = m.lm64(s)
        assert abs(float(v) - want) <= 1e-5 * (abs(want) + 1.0), (s, float(v), want)
        assert int(q) == m.final_state(s), (s, int(q), m.final_state(s))
        h = (m.bos,) + tuple(s)
        for i in range(1, len(h)):       # how deep each token's score backs off: the levels the walk went down
            ctx = h[max(i - (order - 1), 0):i] if order > 1 else ()
            k = 0
            while ctx + (h[i],) not in m.ngrams and ctx:
                ctx = ctx[1:]; k += 1
            depth.add((k, ctx + (h[i],) in m.ngrams))
    assert {k for k, _hit in depth} == set(range(order)), depth       # every back-off depth, 0 .. order - 1
    assert any(not hit for _k, hit in depth) and len({int(q) for q in st}) > (1 if order > 1 else 0)
    assert (st[0], lm[0]) == (m.state_index.get((N,), 0), 0.0)         # the empty string: the start state, lm 0


def test_start_state_without_bos_is_the_empty_context():
    m = MR.Model(4, {(1,): (-1.0, -0.5), (2,): (-2.0, -0.25), (1, 2): (-0.5, 0.0)}, -9.0)
    rc, lm, st, msg = MR.score_call(_lib.load(), m, [(), (1,), (1, 2), (3, 1, 2), (2, 3)])
    assert rc == 0, msg
    assert st.tolist() == [0, 1, 2, 2, 0]
    assert np.allclose(lm, [0.0, -1.0, -1.5, -10.5, -11.25], atol=1e-6)    # (the last: 2, then 2's back-off plus oov)
    assert abs(float(lm[4]) - m.lm64((2, 3))) < 1e-6


# ---------------------------------------------------------------- surface
def test_exports_header_and_python_mirror():
    names = ["rt_lm_create", "rt_lm_info", "rt_set_rec_beam_lm", "rt_rec_beam_lm", "rt_results_rec_beam_lm", "rt_debug_lm_compile",
             "rt_debug_lm_score", "rt_debug_ctc_beam_lm", "rt_debug_ctc_beam_lm_host"]
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n) and ("RT_API" in header and n + "(" in header), n
    assert "#define RT_MAX_LM_ORDER 5" in header and "#define RT_MAX_LM_NGRAMS (1 << 22)" in header and "#define RT_MAX_LMS 4" in header
    assert "typedef struct rt_beam_lm { float lm; float score; } rt_beam_lm;" in header
    assert "has not been measured" in header
    assert (_lib.MAX_LM_ORDER, _lib.MAX_LM_NGRAMS, _lib.MAX_LMS) == (5, 1 << 22, 4) == (MR.MAX_ORDER, MR.MAX_NGRAMS, MR.MAX_LMS)
    assert C.sizeof(_lib.BeamLm) == MR.BEAM_LM.itemsize == 8 and [f[0] for f in _lib.BeamLm._fields_] == list(MR.BEAM_LM.names)
    S = retto_amd.RettoSession
    assert callable(S.create_lm) and callable(S.set_rec_beam_lm) and callable(S.rec_beam_lm) and callable(S.lm_info)
    assert "oov_log10" in inspect.signature(S.create_lm).parameters
    assert list(inspect.signature(S.set_rec_beam_lm).parameters)[1:] == ["lm", "alpha", "beta"]
    h = retto_amd.BeamHypothesis(np.zeros(0, np.int32), "", -1.5)
    assert (h.text, h.logprob, h.lm_logprob, h.lm_score) == ("", -1.5, None, None)
    h = retto_amd.BeamHypothesis(np.zeros(0, np.int32), "", -1.5, -2.0, -3.0)
    assert (h.lm_logprob, h.lm_score) == (-2.0, -3.0)
    # without a session
    assert lib.rt_set_rec_beam_lm(None, 0, 1.0, 0.0) == 8 and b"rt_set_rec_beam_lm: null session" in lib.rt_last_error(None)
    assert lib.rt_rec_beam_lm(None, None, None, None) == 8 and lib.rt_lm_info(None, 0, None, None, None, None) == 8
    assert lib.rt_lm_create(None, b"", 0, -1.0, None) == 8 and lib.rt_results_rec_beam_lm(None, 0, 0, None) == 0
    from retto_amd import cli
    a = cli.build_parser().parse_args(["-i", "x", "--rec-beam", "16,4", "--rec-lm", "m.arpa", "--rec-lm-weights", "0.8,0.6"])
    assert cli.parse_beam(a.rec_beam) == (16, 4) and cli.parse_beam("8") == (8, 1) and cli.parse_weights(a.rec_lm_weights) == (0.8, 0.6)
    assert cli.build_parser().parse_args(["-i", "x"]).rec_beam is None
    for bad in ("", "4,", "a", "1,2,3"):
        with pytest.raises(SystemExit):
            cli.parse_beam(bad)
    with pytest.raises(SystemExit):
        cli.parse_weights("0.8")
    rule = open(os.path.join(ROOT, "retto_amd", "csrc", "ctc_lm.h")).read()
    assert "RT_HD float fused_of(float total, float lm, int len, float alpha, float beta)" in rule
    beam = open(os.path.join(ROOT, "retto_amd", "csrc", "ctc_beam.h")).read()
    assert "language-model fusion," not in beam.split("Out of scope")[1].split("\n//\n")[0]

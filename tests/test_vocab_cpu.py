"""The rec vocabulary (retto_amd/csrc/ctc_vocab.h) without a GPU: the compiler (rt_debug_vocab_compile: UTF-8 words into the id
form, duplicates, case variants and their dropped count, every refusal with its message, the limits); the compiled trie walked on
the host (rt_debug_vocab_walk) against the count by its direct definition in ctc_vocab_ref.py, on strings that reach every row of
the step table; and the surface: exports, header, Python mirror."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import retto_amd
from retto_amd import _lib

import ctc_vocab_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT_BYTES = "a\nb\nc\nd\né\nA\nB\n".encode("utf-8")
DICT = ["blank", "a", "b", "c", "d", "é", "A", "B", " "]     # what the library reads DICT_BYTES as: the blank first, the space last
CLASSES = len(DICT)


def compile_ok(text, **kw):
    rc, got, msg = VR.compile_call(_lib.load(), DICT_BYTES, text, **kw)
    assert rc == 0, msg
    assert got["classes"] == CLASSES
    return got


def walk_ok(vocab, strings, **kw):
    rc, op, cl, st, msg = VR.walk_call(_lib.load(), vocab, strings, **kw)
    assert rc == 0, msg
    n = len(strings)
    return op[:n].tolist(), cl[:n].tolist(), st[:n].tolist()


# ---------------------------------------------------------------- compiler
def test_utf8_words_and_id_words_give_the_same_id_form():
    got = compile_ok("ab\n  cab \r\n\néa\nd")
    words = [(1, 2), (3, 1, 2), (5, 1), (4,)]
    assert got["words"] == words and got["lens"].tolist() == [2, 3, 2, 1] and got["ids"].tolist() == [c for w in words for c in w]
    v = VR.Vocab(CLASSES, words)
    assert (got["n_words"], got["nodes"], got["word_classes"], got["variants_dropped"]) == (4, len(v.node), 5, 0)
    # the same words given as ids compile to the same trie: the walks agree, states included
    strings = [(1, 2), (3, 1), (3, 1, 2, 8, 5), (5, 1, 1), (4, 4), ()]
    a = walk_ok(v, strings)
    b = walk_ok(v, strings, word_form=(got["ids"], got["lens"]))
    assert a == b and a[2] == [v.final_state(s) for s in strings]


def test_a_word_given_twice_is_one_word():
    got = compile_ok("ab\nab\n ab \nb\nab")
    assert got["words"] == [(1, 2), (2,)] and (got["n_words"], got["nodes"]) == (2, 4)
    v = VR.Vocab(CLASSES, [(1, 2), (1, 2), (2,), (1, 2)])          # ... and so it is in the id form of the hooks
    assert walk_ok(v, [(1, 2), (2,), (1,)]) == ([0, 0, 0], [0, 0, 1], [2, 3, 1])


def test_case_variants_and_their_dropped_count():
    plain = compile_ok("ab\ncd\né\nAb\na")
    assert plain["words"] == [(1, 2), (3, 4), (5,), (6, 2), (1,)] and plain["variants_dropped"] == 0
    got = compile_ok("ab\ncd\né\nAb\na", flags=VR.CASE_VARIANTS)
    # ab -> Ab, AB; cd -> Cd, CD: the dictionary has no C (two dropped); é: no ASCII letter; Ab -> (Ab), AB; a -> A, (A)
    assert got["words"] == [(1, 2), (6, 2), (6, 7), (3, 4), (5,), (1,), (6,)]
    assert (got["variants_dropped"], got["n_words"], got["word_classes"]) == (2, 7, 7)
    assert compile_ok("bA\n", flags=VR.CASE_VARIANTS)["words"] == [(2, 6), (7, 6)]     # (Ba = BA here: both B A)


@pytest.mark.parametrize("text,flags,rc,msg", [
    ("ab\nax\n", 0, 8, 'vocab: U+0078 in word 1 ("ax") matches no dictionary entry'),
    ("ab\n\n中\n", 0, 8, 'vocab: U+4E2D in word 1 ("中") matches no dictionary entry'),
    (b"ab\n\xffa\n", 0, 5, "vocab: the text is not valid UTF-8 (byte offset 3)"),
    ("a" * 64, 0, 8, "code points, more than RT_VOCAB_MAX_LEN (63)"),
    ("", 0, 8, "vocab: no word at all"),
    (" \n\r\n", 0, 8, "vocab: no word at all"),
    ("ab", 2, 8, "vocab: unknown flag bits 0x2"),
    ("ab", 5, 8, "vocab: unknown flag bits 0x4"),
])
def test_compiler_refusals_name_the_word(text, flags, rc, msg):
    got_rc, got, err = VR.compile_call(_lib.load(), DICT_BYTES, text, flags=flags)
    assert got_rc == rc and msg in err, (got_rc, err)
    assert got["n"] == 0 and got["nodes"] == 0
    if len(text) == 64:      # (an over-long word is named by its start)
        assert 'word 0 ("' + "a" * 48 + '...") has 64 code points' in err


def test_compiler_caps_and_a_63_id_word():
    got = compile_ok("a" * 63)
    assert got["lens"].tolist() == [63] and got["nodes"] == 64
    rc, got, err = VR.compile_call(_lib.load(), DICT_BYTES, "ab\ncab\n", cap=1)
    assert rc == 8 and "the vocabulary needs 5 ids and 2 words" in err and (got["n"], got["n_ids"], got["n_words"]) == (2, 5, 2)


def test_id_form_refusals_name_the_word():
    lib = _lib.load()
    v = VR.Vocab(5, [(1, 2), (3,)])
    for form, classes, rc, msg in ((([1, 0, 3], [2, 1]), 5, 8, "rt_debug_vocab_walk: vocab: word 0: the blank (class 0) is not a token"),
                                   (([1, 2, 5], [2, 1]), 5, 8, "vocab: word 1: class id 5 is outside [1, 5)"),
                                   (([1, 2, -1], [2, 1]), 5, 8, "vocab: word 1: class id -1 is outside [1, 5)"),
                                   (([1, 2, 3], [3, 0]), 5, 8, "vocab: word 1 is empty"),
                                   (([1] * 64, [64]), 5, 8, "vocab: word 0 has 64 ids, more than RT_VOCAB_MAX_LEN (63)"),
                                   (([], []), 5, 8, "vocab: no word at all"),
                                   (([1], [1]), 1, 8, "vocab: the vocabulary needs at least 2 classes")):
        got, _o, _c, st, err = VR.walk_call(lib, v, [(1,)], word_form=(np.array(form[0], np.int32), np.array(form[1], np.int32)), classes=classes)
        assert got == rc and msg in err, (got, err)
        assert st[0] == VR.CANARY_OOV
    got, _o, _c, st, err = VR.walk_call(lib, v, [(1,), (1, 5)])
    assert got == 8 and "class id 5 in string 1 is outside [1, 5)" in err and st[0] == VR.CANARY_OOV


def test_the_word_limit():
    """RT_VOCAB_MAX_WORDS distinct words compile; one more is RT_ERR_CAPACITY; a word given again does not count"""
    lib = _lib.load()
    n = VR.MAX_WORDS
    k = np.arange(n + 1, dtype=np.int64)
    ids = np.stack([1 + k // 16384, 1 + (k // 128) % 128, 1 + k % 128], axis=1).astype(np.int32)    # (distinct triples over 128 classes)
    v = VR.Vocab(130, [(1,)])
    lens = np.full(n + 1, 3, np.int32)
    rc, op, cl, st, err = VR.walk_call(lib, v, [(1, 1, 1), (1, 1), (129,)], word_form=(ids[:n].ravel(), lens[:n]))
    assert rc == 0 and (op[:3].tolist(), cl[:3].tolist()) == ([0, 0, 0], [0, 1, 0]), err
    again = (np.concatenate([ids[:n].ravel(), ids[0]]), lens)
    assert VR.walk_call(lib, v, [(1,)], word_form=again)[0] == 0
    rc, _o, _c, _s, err = VR.walk_call(lib, v, [(1,)], word_form=(ids.ravel(), lens))
    assert rc == 9 and "more than RT_VOCAB_MAX_WORDS (1048576) words" in err, err


# ---------------------------------------------------------------- the trie, walked
WALK_WORDS = [(1, 2), (1, 2, 3), (2,), (3, 1, 1), (5, 5)]       # (1, 2) is a prefix of (1, 2, 3); classes 4, 6, 7 are separators
WALK_CLASSES = 8


def test_walk_reaches_every_row_of_the_step_table():
    v = VR.Vocab(WALK_CLASSES, WALK_WORDS)
    assert v.word_classes == {1, 2, 3, 5}
    rows = [((), 0, 0, 0),                               # the empty string
            ((4,), 0, 0, 0),                             # a separator at the root: nothing closed
            ((1,), 0, 1, v.node[(1,)]),                  # a line ending in an open prefix: counted only by the line end
            ((1, 4), 1, 1, 0),                           # a separator closes a prefix that is no entry
            ((1, 2), 0, 0, v.node[(1, 2)]),              # an entry that is a prefix of another, open and terminal
            ((1, 2, 4), 0, 0, 0),                        # ... closed by a separator: an entry
            ((1, 2, 3), 0, 0, v.node[(1, 2, 3)]),        # the longer entry
            ((1, 2, 3, 1), 1, 1, VR.OFF),                # a node without such a child: OFF, counted at once
            ((1, 2, 3, 1, 2, 2), 1, 1, VR.OFF),          # OFF through to the line end: counted once
            ((1, 2, 3, 1, 6, 2), 1, 1, v.node[(2,)]),    # OFF, a separator (nothing added again), then an entry
            ((5,), 0, 1, v.node[(5,)]), ((5, 5, 5), 1, 1, VR.OFF),
            ((3,), 0, 1, v.node[(3,)]), ((3, 1), 0, 1, v.node[(3, 1)]), ((3, 2), 1, 1, VR.OFF),
            ((7, 4, 6), 0, 0, 0),                        # separators only
            ((2, 4, 2, 7, 1, 6, 3, 3), 2, 2, VR.OFF)]    # several words: 2 ok, 2 ok, (1) none, (3, 3) none
    op, cl, st = walk_ok(v, [r[0] for r in rows])
    for (s, o, c, state), go, gc, gs in zip(rows, op, cl, st):
        assert (go, gc, gs) == (o, c, state) == (v.count(s, closed=False), v.count(s), v.final_state(s)), (s, go, gc, gs)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_walk_against_the_definition_on_seeded_strings(seed):
    rng = np.random.default_rng(7700 + seed)
    classes = (6, 40, 300)[seed]
    real = [c for c in range(1, classes) if c % 4]
    words = [tuple(int(real[int(i)]) for i in rng.integers(0, len(real), int(rng.integers(1, 7)))) for _ in range(60)]
    words += [w[:k] for w in words[:20] for k in (1, 2) if len(w) > k]               # prefixes of entries as entries
    v = VR.Vocab(classes, words)
    strings = []
    for _ in range(400):
        s = []
        for _ in range(int(rng.integers(0, 5))):
            w = words[int(rng.integers(len(words)))]
            kind = int(rng.integers(4))
            w = w if kind == 0 else w[:max(1, len(w) - 1)] if kind == 1 else w + (int(real[int(rng.integers(len(real)))]),) if kind == 2 else \
                tuple(int(x) for x in rng.integers(1, classes, 3))
            s += list(w) + ([int(4 * rng.integers(1, (classes + 3) // 4))] if rng.random() < 0.8 else [])
        strings.append(tuple(c for c in s if 1 <= c < classes))
    op, cl, st = walk_ok(v, strings)
    assert op == [v.count(s, closed=False) for s in strings]
    assert cl == [v.count(s) for s in strings]
    assert st == [v.final_state(s) for s in strings]
    assert any(a != b for a, b in zip(op, cl)) and VR.OFF in st and 0 in st and max(cl) >= 3


# ---------------------------------------------------------------- surface
def test_exports_header_and_python_mirror():
    names = ["rt_vocab_create", "rt_vocab_info", "rt_set_rec_beam_vocab", "rt_rec_beam_vocab", "rt_results_rec_beam_vocab",
             "rt_debug_vocab_compile", "rt_debug_vocab_walk", "rt_debug_ctc_beam_vocab", "rt_debug_ctc_beam_vocab_host"]
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "retto_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n) and ("RT_API" in header and n + "(" in header), n
    assert "#define RT_VOCAB_MAX_LEN 63" in header and "#define RT_VOCAB_MAX_WORDS (1 << 20)" in header and "#define RT_MAX_VOCABS 4" in header
    assert "#define RT_VOCAB_CASE_VARIANTS 1" in header
    assert "typedef struct rt_beam_vocab { int32_t oov_words; float score; } rt_beam_vocab;" in header
    assert "has not been measured" in header.split("rec vocabulary")[1]
    assert (_lib.VOCAB_MAX_LEN, _lib.VOCAB_MAX_WORDS, _lib.MAX_VOCABS, _lib.VOCAB_CASE_VARIANTS) == (63, 1 << 20, 4, 1) == \
        (VR.MAX_LEN, VR.MAX_WORDS, VR.MAX_VOCABS, VR.CASE_VARIANTS)
    assert C.sizeof(_lib.BeamVocab) == VR.BEAM_VOCAB.itemsize == 8 and [f[0] for f in _lib.BeamVocab._fields_] == list(VR.BEAM_VOCAB.names)
    S = retto_amd.RettoSession
    assert callable(S.create_vocab) and callable(S.set_rec_beam_vocab) and callable(S.rec_beam_vocab) and callable(S.vocab_info)
    assert list(inspect.signature(S.create_vocab).parameters)[1:] == ["words", "ids", "case_variants"]
    assert list(inspect.signature(S.set_rec_beam_vocab).parameters)[1:] == ["vocab", "gamma"]
    assert inspect.signature(S.set_rec_beam_vocab).parameters["gamma"].default == 4.0
    h = retto_amd.BeamHypothesis(np.zeros(0, np.int32), "", -1.5)
    assert (h.lm_score, h.oov_words, h.vocab_score) == (None, None, None)
    h = retto_amd.BeamHypothesis(np.zeros(0, np.int32), "", -1.5, None, None, 2, -9.5)
    assert (h.oov_words, h.vocab_score) == (2, -9.5)
    # without a session
    assert lib.rt_set_rec_beam_vocab(None, 0, 1.0) == 8 and b"rt_set_rec_beam_vocab: null session" in lib.rt_last_error(None)
    assert lib.rt_rec_beam_vocab(None, None, None) == 8 and lib.rt_vocab_info(None, 0, None, None, None, None) == 8
    assert lib.rt_vocab_create(None, b"", 0, None, None, 0, 0, None) == 8 and lib.rt_results_rec_beam_vocab(None, 0, 0, None) == 0
    from retto_amd import cli
    a = cli.build_parser().parse_args(["-i", "x", "--rec-beam", "16,4", "--rec-vocab", "w.txt", "--rec-vocab-gamma", "2.5", "--rec-vocab-case-variants"])
    assert (a.rec_vocab, a.rec_vocab_gamma, a.rec_vocab_case_variants) == ("w.txt", 2.5, True)
    a = cli.build_parser().parse_args(["-i", "x"])
    assert (a.rec_vocab, a.rec_vocab_gamma, a.rec_vocab_case_variants) == (None, 4.0, False)
    rule = open(os.path.join(ROOT, "retto_amd", "csrc", "ctc_vocab.h")).read()
    assert "RT_HD Step step(const View& v, int state, int c)" in rule and "RT_HD float key_of(float total, float fused, int oov, float gamma)" in rule
    for f in ("ctc_lm.h", "ctc_beam.h"):     # word lists are no longer out of scope there; per-region ones and word-level n-grams are
        scope = open(os.path.join(ROOT, "retto_amd", "csrc", f)).read().split("Out of scope")[1].split("\n#pragma")[0].split("\n//\n")[0]
        assert "word-level n-grams" in scope and "word-level or neural" not in scope, f

"""The rec tail's text front end (retto_amd/csrc/rec_text.h: the strict UTF-8 decoder, the trimmed-line reader, the table of
one-code-point classes, the dictionary loader and the charset, lexicon and vocabulary compilers) under AddressSanitizer + UBSan:
a stand-alone driver (tests/native/rec_text_driver.cpp, run as a program; nothing is loaded into Python under a sanitizer) reads
every case from exactly sized heap buffers, so a read past the end of the text is an error, and must answer what the library's
rt_debug_*_compile hooks answer on the same bytes: the code, the message and the arrays.  Exit code 0 and an empty stderr
throughout.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from retto_amd import _lib
from oracle.pipeline import load_dictionary

import ctc_vocab_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# classes: 0 blank, 1 a, 2 b, 3 c, 4 A, 5 B, 6 e-acute, 7 U+4E2D, 8 U+1F600, 9 "0", 10 the appended " "
DICT = "a\nb\nc\nA\nB\né\n中\n\U0001F600\n0\n".encode()
DUPS = b"a\nb\na\nb\nc\n"                                   # a: 1 and 3, b: 2 and 4, c: 5

# (name, dictionary, text, vocab flags)
CASES = [
    ("ordinary", DICT, "abc\nba\n中é\U0001F600\n".encode(), 0),
    ("charset_text", DICT, "abc中\U0001F600 0".encode(), 0),
    ("crlf", DICT, b"ab\r\nc\r\nba\r", 0),                   # (the last \r is no line end: trimmed as whitespace)
    ("lone_cr", DICT, b"ab\nc\rb\n", 0),                     # (a \r that is not before \n stays in its line: U+000D)
    ("u3000_lines", DICT, "ab\n　　\n　c　\n".encode(), 0),
    ("empty_lines", DICT, b"ab\n\n\nc\n\n", 0),
    ("no_final_newline", DICT, b"ab\n\nc", 0),
    ("empty_text", DICT, b"", 0),
    ("cut_2", DICT, b"ab\n\xc3", 0),
    ("cut_3", DICT, b"ab\n\xe4\xb8", 0),
    ("cut_3_lead", DICT, b"ab\n\xe4", 0),
    ("cut_4", DICT, b"ab\n\xf0\x9f\x98", 0),
    ("cut_4_lead", DICT, b"ab\n\xf0", 0),
    ("overlong_2", DICT, b"a\xc0\xaf\n", 0),
    ("overlong_3", DICT, b"ab\nc\xe0\x80\xaf\n", 0),
    ("surrogate", DICT, b"ab\n\xed\xa0\x80\n", 0),
    ("above_10ffff", DICT, b"\xf4\x90\x80\x80", 0),
    ("missing", DICT, b"ab\nabz\n", 0),
    ("duplicates", DUPS, b"ab\nc\nba", 0),
    ("case_variants", DICT, b"ab\nabc\nAb\n0\n", 1),         # (ABC lacks C: one variant dropped)
    ("unknown_flags", DICT, b"ab\n", 6),
]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rec_text_driver") / "rec_text_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), os.path.join(ROOT, "tests", "native", "rec_text_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the rec text driver does not build:\n" + r.stderr[-3000:]
    return out


def run(exe, tmp_path, op, dictionary, text=None, flags=None):
    """-> ({rc, classes, ...} as ints, message, the rows behind the first line as lists of words)"""
    args = [exe, op, str(tmp_path / "dict.bin")]
    open(args[2], "wb").write(dictionary)
    if text is not None:
        args.append(str(tmp_path / "text.bin"))
        open(args[3], "wb").write(text)
    if flags is not None:
        args.append(str(flags))
    r = subprocess.run(args, capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.decode("utf-8", "replace").split("\n")
    head, msg = lines[0].split(" msg=", 1)
    return {k: int(v) for k, v in (kv.split("=") for kv in head.split())}, msg, [l.split() for l in lines[1:-1]]


def ints(row):
    return [int(x) for x in row]


def lib_charset(lib, dictionary, text):
    mask = np.zeros(8, np.uint32)
    n, err = C.c_int(), C.create_string_buffer(512)
    rc = lib.rt_debug_charset_compile(dictionary, len(dictionary), text, len(text), None, 0, mask.ctypes.data, len(mask), C.byref(n), err, 512)
    return rc, n.value, err.value.decode("utf-8", "replace"), mask[:(n.value + 31) // 32 if rc == 0 else 0].tolist()


def lib_lexicon(lib, dictionary, text):
    ids, lens = np.zeros(256, np.int32), np.zeros(64, np.int32)
    ni, ne, nc, err = C.c_int(), C.c_int(), C.c_int(), C.create_string_buffer(512)
    rc = lib.rt_debug_lexicon_compile(dictionary, len(dictionary), text, len(text), None, None, 0, ids.ctypes.data, len(ids), lens.ctypes.data,
                                      len(lens), C.byref(ni), C.byref(ne), C.byref(nc), err, 512)
    return rc, nc.value, err.value.decode("utf-8", "replace"), ids[:ni.value].tolist(), lens[:ne.value].tolist()


@pytest.mark.parametrize("name,dictionary,text,flags", CASES, ids=IDS)
def test_driver_answers_what_the_library_hooks_answer(exe, tmp_path, name, dictionary, text, flags):
    lib = _lib.load()
    got, msg, rows = run(exe, tmp_path, "charset", dictionary, text)
    rc, classes, want_msg, mask = lib_charset(lib, dictionary, text)
    assert (got["rc"], got["classes"], msg, ints(rows[0])) == (rc, classes, want_msg, mask)

    got, msg, rows = run(exe, tmp_path, "lexicon", dictionary, text)
    rc, classes, want_msg, ids, lens = lib_lexicon(lib, dictionary, text)
    assert (got["rc"], got["classes"], msg, ints(rows[0]), ints(rows[1])) == (rc, classes, want_msg, ids, lens)

    got, msg, rows = run(exe, tmp_path, "vocab", dictionary, text, flags)
    rc, out, want_msg = VR.compile_call(lib, dictionary, text, flags)
    assert (got["rc"], got["classes"], msg, ints(rows[0]), ints(rows[1])) == (rc, out["classes"], want_msg, out["ids"].tolist(), out["lens"].tolist())
    assert (got["words"], got["nodes"], got["word_classes"], got["variants_dropped"]) == \
        (out["n_words"], out["nodes"], out["word_classes"], out["variants_dropped"])


@pytest.mark.parametrize("name,dictionary,text,flags", CASES, ids=IDS)
def test_every_text_read_as_a_dictionary(exe, tmp_path, name, dictionary, text, flags):
    """the case's text through the loader: the driver's entries are the Python restatement's, and its refusal the library's"""
    lib = _lib.load()
    got, msg, rows = run(exe, tmp_path, "dict", text)
    rc, classes, want_msg, _mask = lib_charset(lib, text, b"")
    assert (got["rc"], got["classes"], msg) == (rc, classes, want_msg)
    if rc == 0:
        want = load_dictionary(text)
        assert got["classes"] == len(want)
        assert [b"" if e == "-" else bytes.fromhex(e) for e in rows[0]] == [e.encode() for e in want]
    else:
        assert rc == 5 and rows == [[]]


def test_the_rules_themselves(exe, tmp_path):
    """what the cases are there for, stated: so that the two sides cannot agree on a wrong answer"""
    by = {c[0]: c for c in CASES}
    lex = lambda name: run(exe, tmp_path, "lexicon", by[name][1], by[name][2])
    assert lex("ordinary")[2] == [["1", "2", "3", "2", "1", "7", "6", "8"], ["3", "2", "3"]]
    for name in ("crlf", "u3000_lines", "empty_lines", "no_final_newline"):              # ab / c (/ ba): nothing else opens an entry
        got, msg, rows = lex(name)
        assert got["rc"] == 0 and rows[0][:3] == ["1", "2", "3"] and rows[1][:2] == ["2", "1"] and len(rows[1]) == (3 if name == "crlf" else 2)
    assert lex("lone_cr")[:2] == ({"rc": 8, "classes": 11}, "lexicon: U+000D in entry 1 matches no dictionary entry")
    assert lex("missing")[:2] == ({"rc": 8, "classes": 11}, "lexicon: U+007A in entry 1 matches no dictionary entry")
    assert lex("empty_text")[:2] == ({"rc": 8, "classes": 11}, "lexicon: no entry")
    for name, off in (("cut_2", 3), ("cut_3", 3), ("cut_3_lead", 3), ("cut_4", 3), ("cut_4_lead", 3), ("overlong_2", 1), ("overlong_3", 4),
                      ("surrogate", 3), ("above_10ffff", 0)):
        assert lex(name)[:2] == ({"rc": 5, "classes": 11}, "lexicon: the text is not valid UTF-8 (byte offset %d)" % off)
        got, msg, rows = run(exe, tmp_path, "vocab", by[name][1], by[name][2], 0)
        assert (got["rc"], msg, rows) == (5, "vocab: the text is not valid UTF-8 (byte offset %d)" % off, [[], []])
        got, msg, rows = run(exe, tmp_path, "dict", by[name][2])
        assert (got["rc"], got["classes"], msg) == (5, 0, "dictionary is not valid UTF-8 (byte offset %d)" % off)
    # duplicate entries: the lowest id wins in a lexicon and a vocabulary, all join in a charset
    assert lex("duplicates")[2] == [["1", "2", "5", "2", "1"], ["2", "1", "2"]]
    assert run(exe, tmp_path, "vocab", DUPS, by["duplicates"][2], 0)[2] == [["1", "2", "5", "2", "1"], ["2", "1", "2"]]
    assert run(exe, tmp_path, "charset", DUPS, b"ab")[2] == [[str(0b11111)]]
    assert run(exe, tmp_path, "charset", DICT, by["charset_text"][2])[2] == [[str(0b11110001111)]]
    # CASE_VARIANTS: ab Ab AB / abc Abc (ABC dropped) / Ab seen / 0 has no letter
    got, msg, rows = run(exe, tmp_path, "vocab", DICT, by["case_variants"][2], 1)
    assert (got["rc"], got["variants_dropped"], got["words"]) == (0, 1, 6)
    assert rows == [["1", "2", "4", "2", "4", "5", "1", "2", "3", "4", "2", "3", "9"], ["2", "2", "2", "3", "3", "1"]]
    assert run(exe, tmp_path, "vocab", DICT, b"ab\n", 6)[:2] == \
        ({"rc": 8, "classes": 11, "words": 0, "nodes": 0, "word_classes": 0, "variants_dropped": 0}, "vocab: unknown flag bits 0x6")
    # the dictionary's own rule: an empty line in the middle is an entry, a trailing \n opens none, one \r before \n is dropped
    assert run(exe, tmp_path, "dict", b"a\n\nb\r\n\r\r\n")[2] == [[b"blank".hex(), "61", "-", "62", "-", "20"]]

"""The rec vocabulary's compiler and walk (retto_amd/csrc/ctc_vocab.h) and the host beam rule with a word list (ctc_host_ref.h)
under AddressSanitizer + UBSan: a stand-alone driver (tests/native/vocab_driver.cpp, run as a program; nothing is loaded into
Python under a sanitizer) compiles seeded and malformed id forms over exactly sized buffers, walks strings and steps from every
state, those outside the trie included, and runs hr::BeamVocabArgs' check and hr::beam_vocab_ref on test_ctc_host_driver_cpu.py's
shapes -- N = 9 classes, lines of 0, 1, 2, 7 and 40 time steps -- whose outputs must be the bytes of the library's
rt_debug_ctc_beam_vocab_host.  Every input ends in a status code: exit code 0 and an empty stderr throughout.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lm_ref as MR
import ctc_vocab_ref as VR
from test_ctc_host_driver_cpu import D, N, TPL, f32, head, i32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vocab_driver") / "vocab_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), os.path.join(ROOT, "tests", "native", "vocab_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the vocab driver does not build:\n" + r.stderr[-3000:]
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout.strip()


def fields(line):
    head_, msg = line.split(" msg=", 1)
    return dict(kv.split("=") for kv in head_.split()), msg


def words_file(path, classes, ids, lens):
    open(path, "wb").write(b"".join(np.ascontiguousarray(p).tobytes() for p in (i32([classes, len(lens)]), i32(lens), i32(ids))))
    return path


def test_seeded_vocabularies_compile_to_the_trie(exe, tmp_path):
    rng = np.random.default_rng(7800)
    for classes, n in ((5, 1), (9, 30), (300, 400)):
        words = [tuple(int(c) for c in rng.integers(1, min(classes, 6), int(rng.integers(1, 8)))) for _ in range(n)]
        words += [w[:1] for w in words[:5]] + words[:3]          # (prefixes as entries; words given twice)
        v = VR.Vocab(classes, words)
        got, msg = fields(run(exe, "words", words_file(str(tmp_path / "w.bin"), classes, *v.id_form())))
        assert msg == "" and int(got["rc"]) == 0
        assert (int(got["words"]), int(got["nodes"]), int(got["arcs"]), int(got["word_classes"])) == \
            (len(v.entries), len(v.node), len(v.node) - 1, len(v.word_classes))


def test_refusals_carry_their_message(exe, tmp_path):
    p = str(tmp_path / "bad.bin")
    for classes, ids, lens, rc, want in ((5, [1, 0], [2], 8, "vocab: word 0: the blank (class 0) is not a token"),
                                         (5, [1, 2, 7], [2, 1], 8, "vocab: word 1: class id 7 is outside [1, 5)"),
                                         (5, [1, 2], [2, 0], 8, "vocab: word 1 is empty"),
                                         (5, [1, 2], [2, -3], 8, "vocab: word 1 is empty"),
                                         (5, [1] * 64, [64], 8, "vocab: word 0 has 64 ids, more than RT_VOCAB_MAX_LEN (63)"),
                                         (5, [], [], 8, "vocab: no word at all"),
                                         (1, [1], [1], 8, "vocab: the vocabulary needs at least 2 classes (the blank and one class)")):
        got, msg = fields(run(exe, "words", words_file(p, classes, ids, lens)))
        assert int(got["rc"]) == rc and msg == want and int(got["nodes"]) == 0, (got, msg)


@pytest.mark.parametrize("classes,seed", [(2, 1), (5, 2), (40, 3), (6625, 4)])
def test_seeded_and_malformed_id_forms(exe, classes, seed):
    out = run(exe, "fuzz", classes, 2000 + seed, 400)
    ok, refused = (int(kv.split("=")[1]) for kv in out.split())
    assert ok + refused == 400 and ok >= 100 and refused >= 100, out


def beam_input(z, W, b, tpl, beam, nbest, v, gamma, m, alpha, beta, out, word_form=None):
    none = (i32([]), i32([]), f32([]), f32([]))
    ids, lens, logp, bo = none if m is None else m.id_form()
    wids, wlens = v.id_form() if word_form is None else word_form
    parts = [i32([W.shape[1], len(tpl), beam, nbest, len(lens), len(wlens)]), f32([0.0 if m is None else m.oov, alpha, beta, gamma]), i32(tpl), i32(lens),
             i32(wlens), i32(ids), f32(logp), f32(bo), i32(wids), f32(z), f32(W), f32(b), out["n"][:len(tpl)], out["beams"][:len(tpl)],
             out["tokens"][:sum(max(t, 0) for t in tpl) * nbest], out["lm"][:len(tpl)], out["vocab"][:len(tpl)]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def driver_vocab(z, W, b):
    texts = [R[0][0] for _lp, R in BR.reference(z, W, b, TPL, 4) if R]
    rng = np.random.default_rng(7900)
    words = [tuple(c for c in t[:k] if c % 4) for t in texts for k in (2, len(t)) if any(c % 4 for c in t[:k])]
    words += [tuple(int(c) for c in rng.choice([1, 2, 3, 5, 6, 7], int(rng.integers(1, 5)))) for _ in range(8)]
    return texts, VR.Vocab(N, words)


@pytest.mark.parametrize("fused", [False, True], ids=["alone", "with_model"])
@pytest.mark.parametrize("beam,nbest", [(1, 1), (4, 4), (32, 8)])
def test_host_rule_is_the_library_entry_bit_for_bit(exe, tmp_path, fused, beam, nbest):
    z, W, b = head(TPL)
    assert (z.shape[1], W.shape) == (D, (D, N))
    texts, v = driver_vocab(z, W, b)
    m = MR.random_model(53, N, 3, texts, per_level=80) if fused else None
    al, be = (MR.ALPHA, MR.BETA) if fused else (0.0, 0.0)
    rc, want = VR.call(_lib.load().rt_debug_ctc_beam_vocab_host, None, z, W, b, TPL, beam, nbest, v, VR.GAMMA, m, al, be)
    assert rc == 0 and want["n"].tolist() == [0] + [min(nbest, k) for k in want["n"][1:]]
    inp, outp = str(tmp_path / "beam.in"), str(tmp_path / "beam.out")
    open(inp, "wb").write(beam_input(z, W, b, TPL, beam, nbest, v, VR.GAMMA, m, al, be, VR.new_outputs(TPL, nbest)))
    assert run(exe, "beam", inp, outp) == "ok"
    rows = sum(TPL)
    got = open(outp, "rb").read()
    assert got == b"".join(want[k][:n].tobytes() for k, n in (("n", len(TPL)), ("beams", len(TPL)), ("tokens", rows * nbest), ("lm", len(TPL)),
                                                              ("vocab", len(TPL))))
    hyps = VR.hyps_of(want, TPL, nbest, fused)
    assert all(int(h[4]) == v.count(h[0]) for H in hyps for h in H) and any(int(h[4]) > 0 for H in hyps for h in H)


def test_refused_calls_write_nothing(exe, tmp_path):
    lib = _lib.load()
    z, W, b = head(TPL)
    v = VR.Vocab(N, [(1, 2), (3,)])
    wids, wlens = v.id_form()
    inp, outp = str(tmp_path / "bad.in"), str(tmp_path / "bad.out")
    for kw, want in ((dict(gamma=-1.0), "gamma is not a finite number at least 0"), (dict(gamma=float("inf")), "gamma is not a finite number at least 0"),
                     (dict(word_form=(i32([1, 0, 3]), wlens)), "vocab: word 0: the blank (class 0) is not a token"),
                     (dict(word_form=(i32([1, 2, 9]), wlens)), "vocab: word 1: class id 9 is outside [1, 9)"),
                     (dict(word_form=(i32([]), i32([]))), "vocab: no word at all"),
                     (dict(beam=33), "beam = 33 is outside [0, RT_MAX_BEAM]")):
        a = dict(beam=4, gamma=1.0, word_form=None)
        a.update(kw)
        fresh = VR.new_outputs(TPL, 2)
        blob = beam_input(z, W, b, TPL, a["beam"], 2, v, a["gamma"], None, 0.0, 0.0, fresh, word_form=a["word_form"])
        open(inp, "wb").write(blob)
        assert run(exe, "beam", inp, outp) == "error: " + want
        assert blob.endswith(open(outp, "rb").read())     # (the outputs as they went in)
        rc, _out = VR.call(lib.rt_debug_ctc_beam_vocab_host, None, z, W, b, TPL, a["beam"], 2, v, a["gamma"], word_form=a["word_form"])
        assert rc == 8 and lib.rt_last_error(None).decode() == "rt_debug_ctc_beam_vocab_host: " + want

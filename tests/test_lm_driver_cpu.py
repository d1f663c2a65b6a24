"""The rec language model's parser, compiler and walk (retto_amd/csrc/ctc_lm.h) and the host beam rule with fusion
(ctc_host_ref.h) under AddressSanitizer + UBSan: a stand-alone driver (tests/native/lm_driver.cpp, run as a program; nothing is
loaded into Python under a sanitizer) compiles valid, truncated and byte-mutated ARPA files over exactly sized buffers, and runs
hr::BeamLmArgs' check and hr::beam_lm_ref on test_ctc_host_driver_cpu.py's shapes -- N = 9 classes, lines of 0, 1, 2, 7 and 40
time steps -- whose outputs must be the bytes of the library's rt_debug_ctc_beam_lm_host.  Exit code 0 and an empty stderr
throughout.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from retto_amd import _lib

import ctc_beam_ref as BR
import ctc_lm_ref as MR
from test_ctc_host_driver_cpu import D, N, TPL, f32, head, i32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT = ["blank", "a", "b", "c", "d", "é", " "]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lm_driver") / "lm_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "retto_amd", "csrc"), os.path.join(ROOT, "tests", "native", "lm_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the lm driver does not build:\n" + r.stderr[-3000:]
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout.strip()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lm_files")
    dic = str(d / "dict.txt")
    open(dic, "wb").write("\n".join(DICT[1:-1]).encode("utf-8"))
    models = {}
    for order in (1, 3, 5):
        m = MR.random_model(30 + order, len(DICT), order, texts=[(1, 6, 5, 2, 1), (6, 6, 1), (5, 5, 6, 2)])
        path = str(d / ("m%d.arpa" % order))
        open(path, "wb").write(MR.write_arpa(m, DICT, unk=-5.5 if order == 3 else None,
                                             extra=((1, "-1.0\tzz"), (1, "-2.0\t</s>")) if order == 5 else ()).encode("utf-8"))
        models[order] = (m, path)
    return dic, models, d


def fields(line):
    head_, msg = line.split(" msg=", 1)
    return dict(kv.split("=") for kv in head_.split()), msg


@pytest.mark.parametrize("order", [1, 3, 5])
def test_valid_files_compile_to_the_model(exe, files, order):
    dic, models, _d = files
    m, path = models[order]
    got, msg = fields(run(exe, "arpa", dic, path, -6.5))
    assert msg == "" and int(got["rc"]) == 0
    assert (int(got["n"]), int(got["order"]), int(got["states"])) == (len(m.grams), order, len(m.state_index))
    assert int(got["dropped"]) == (2 if order == 5 else 0) and int(got["arcs"]) == sum(1 for g in m.grams if len(g) > 1)
    assert int(got["start"]) == m.state_index.get((len(DICT),), 0)
    assert np.float32(got["oov"]) == np.float32((-5.5 if order == 3 else np.float64(np.float32(-6.5))) * MR.LN10)


def test_refusals_carry_their_message(exe, files):
    dic, _models, d = files
    bad = str(d / "bad.arpa")
    for text, want in (("\\data\\\nngram 1=1\n\n\\1-grams:\nnan\ta\n\\end\\\n", "lm: line 5: a number is not finite"),
                       ("\\data\\\nngram 1=1\n\n\\1-grams:\n-1\ta\n", "the file ends without \\end\\"), ("", "no \\data\\ section")):
        open(bad, "wb").write(text.encode("utf-8"))
        got, msg = fields(run(exe, "arpa", dic, bad, -6.5))
        assert int(got["rc"]) == 8 and want in msg, (got, msg)


@pytest.mark.parametrize("order", [1, 3, 5])
def test_truncated_and_mutated_files(exe, files, order):
    dic, models, _d = files
    out = run(exe, "fuzz", dic, models[order][1], -6.5, 1000 + order, 300)
    ok, refused = (int(kv.split("=")[1]) for kv in out.split())
    assert ok + refused == 600 and refused >= 300 and ok >= 10, out    # (every truncation is refused; some mutations still parse)


def beam_input(z, W, b, tpl, beam, nbest, m, alpha, beta, out, id_form=None):
    ids, lens, logp, bo = m.id_form() if id_form is None else id_form
    parts = [i32([W.shape[1], len(tpl), beam, nbest, len(lens)]), f32([m.oov, alpha, beta]), i32(tpl), i32(lens), i32(ids), f32(logp), f32(bo),
             f32(z), f32(W), f32(b), out["n"][:len(tpl)], out["beams"][:len(tpl)], out["tokens"][:sum(max(t, 0) for t in tpl) * nbest], out["lm"][:len(tpl)]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.mark.parametrize("order", [3, 5])
@pytest.mark.parametrize("beam,nbest", [(1, 1), (4, 4), (32, 8)])
def test_host_rule_is_the_library_entry_bit_for_bit(exe, files, order, beam, nbest):
    _dic, _models, d = files
    z, W, b = head(TPL)
    assert (z.shape[1], W.shape) == (D, (D, N))
    texts = [R[0][0] for _lp, R in BR.reference(z, W, b, TPL, 4) if R]
    m = MR.random_model(50 + order, N, order, texts, per_level=80)
    rc, want = MR.call(_lib.load().rt_debug_ctc_beam_lm_host, None, z, W, b, TPL, beam, nbest, m, MR.ALPHA, MR.BETA)
    assert rc == 0 and want["n"].tolist() == [0] + [min(nbest, k) for k in want["n"][1:]]
    inp, outp = str(d / "beam.in"), str(d / "beam.out")
    open(inp, "wb").write(beam_input(z, W, b, TPL, beam, nbest, m, MR.ALPHA, MR.BETA, MR.new_outputs(TPL, nbest)))
    assert run(exe, "beam", inp, outp) == "ok"
    rows = sum(TPL)
    got = open(outp, "rb").read()
    assert got == b"".join(want[k][:n].tobytes() for k, n in (("n", len(TPL)), ("beams", len(TPL)), ("tokens", rows * nbest), ("lm", len(TPL))))
    MR.hyps_of(want, TPL, nbest)


def test_refused_calls_write_nothing(exe, files):
    _dic, _models, d = files
    lib = _lib.load()
    z, W, b = head(TPL)
    m = MR.Model(N, {(1,): (-1.0, -0.5), (2,): (-1.0, -0.5), (1, 2): (-0.5, 0.0)}, -9.0)
    _ids, lens, logp, bo = m.id_form()
    inp, outp = str(d / "bad.in"), str(d / "bad.out")
    for kw, want in ((dict(alpha=-1.0), "alpha is not a finite number at least 0"), (dict(beta=float("inf")), "beta is not finite"),
                     (dict(id_form=(i32([1, 0, 1, 2]), lens, logp, bo)), "lm: n-gram 1: the blank (class 0) is not a token"),
                     (dict(id_form=(i32([1, 2, 3, 2]), lens, logp, bo)), "lm: n-gram 2: the n-gram's context (its first 1 tokens) is not an n-gram"),
                     (dict(beam=33), "beam = 33 is outside [0, RT_MAX_BEAM]")):
        a = dict(beam=4, alpha=0.5, beta=0.5, id_form=None)
        a.update(kw)
        fresh = MR.new_outputs(TPL, 2)
        blob = beam_input(z, W, b, TPL, a["beam"], 2, m, a["alpha"], a["beta"], fresh, id_form=a["id_form"])
        open(inp, "wb").write(blob)
        assert run(exe, "beam", inp, outp) == "error: " + want
        assert blob.endswith(open(outp, "rb").read())     # (the outputs as they went in)
        rc, _out = MR.call(lib.rt_debug_ctc_beam_lm_host, None, z, W, b, TPL, a["beam"], 2, m, a["alpha"], a["beta"], id_form=a["id_form"])
        assert rc == 8 and lib.rt_last_error(None).decode() == "rt_debug_ctc_beam_lm_host: " + want

"""bench.py's command line without a GPU: `--steps` is the number of timed steps as given, and `--dump-outputs` writes
what a results handle holds as float32 / float64 .npy files, capped in size by a seeded sample of lines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, r.stderr[-1500:]


def test_full_is_opt_in(monkeypatch):
    """A plain run leaves every leg beyond the headline to --full; --profile-all prints a table of --full's profile pass."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--profile-all"])
    assert bench.parse().full is True
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--profile-all"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--profile-all needs --full" in r.stderr, r.stderr[-1500:]


class _FakeResults:
    """The rt_results_* accessors bench.dump_outputs calls, over numpy arrays: handle r, page i, line k."""

    def __init__(self, handles):
        self.h = handles   # handle -> list of pages; page = dict of per-line arrays + "tokens" (list of int32 arrays)

    def rt_results_count(self, r, i):
        return len(self.h[r][i]["boxes"])

    def _f32(self, r, i, key):
        return self.h[r][i][key].ctypes.data_as(C.POINTER(C.c_float))

    def rt_results_boxes(self, r, i):
        return self._f32(r, i, "boxes")

    def rt_results_det_scores(self, r, i):
        return self._f32(r, i, "det")

    def rt_results_cls_scores(self, r, i):
        return self._f32(r, i, "cls")

    def rt_results_rec_scores(self, r, i):
        return self._f32(r, i, "rec")

    def rt_results_cls_labels(self, r, i):
        return self.h[r][i]["labels"].ctypes.data_as(C.POINTER(C.c_uint16))

    def rt_results_rec_tokens(self, r, i, k, ref):
        t = self.h[r][i]["tokens"][k]
        C.cast(C.pointer(ref._obj), C.POINTER(C.c_void_p))[0] = t.ctypes.data if len(t) else None
        return len(t)

    def rt_results_det_checksum(self, r):
        return 1000.0 + r + 0.125


def _page(rng, n):
    return {"boxes": rng.uniform(0, 960, (n, 8)).astype(np.float32), "det": rng.uniform(0, 1, n).astype(np.float32),
            "cls": rng.uniform(0, 1, n).astype(np.float32), "rec": rng.uniform(0, 1, n).astype(np.float32),
            "labels": rng.integers(0, 2, n).astype(np.uint16),
            "tokens": [rng.integers(1, 6625, int(rng.integers(0, 9))).astype(np.int32) for _ in range(n)]}


def test_dump_outputs_writes_every_line_in_page_order(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    lib = _FakeResults({0: [_page(rng, 3), _page(rng, 0), _page(rng, 5)], 1: [_page(rng, 2)]})
    info = bench.dump_outputs(lib, [(0, 3), (1, 1)], str(tmp_path / "out"))
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in info["files"]}
    assert sorted(got) == ["boxes", "cls_labels", "cls_scores", "det_checksum", "det_scores", "line_index", "lines_per_page",
                           "rec_scores", "rec_tokens"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    pages = lib.h[0] + lib.h[1]
    assert info["lines"] == info["lines_written"] == 10
    assert got["lines_per_page"].tolist() == [3, 0, 5, 2] and got["line_index"].tolist() == list(range(10))
    assert got["det_checksum"].tolist() == [1000.125, 1001.125]
    assert np.array_equal(got["boxes"], np.concatenate([p["boxes"] for p in pages]))
    assert np.array_equal(got["cls_labels"], np.concatenate([p["labels"] for p in pages]).astype(np.float32))
    for key, name in (("det", "det_scores"), ("cls", "cls_scores"), ("rec", "rec_scores")):
        assert np.array_equal(got[name], np.concatenate([p[key] for p in pages]))
    toks = [t for p in pages for t in p["tokens"]]
    assert got["rec_tokens"].shape == (10, max(len(t) for t in toks))
    for row, t in zip(got["rec_tokens"], toks):
        assert row[:len(t)].tolist() == t.tolist() and (row[len(t):] == -1).all()


def test_dump_outputs_samples_lines_beyond_the_limit(tmp_path, monkeypatch):
    import bench
    rng = np.random.default_rng(4)
    lib = _FakeResults({0: [_page(rng, 40) for _ in range(5)]})
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    runs = [bench.dump_outputs(lib, [(0, 5)], str(tmp_path / d)) for d in ("a", "b")]
    assert runs[0]["lines"] == 200 and 0 < runs[0]["lines_written"] < 200 and runs[0]["bytes"] <= 4096
    idx_a, idx_b = (np.load(tmp_path / d / "line_index.npy") for d in ("a", "b"))
    assert np.array_equal(idx_a, idx_b) and (np.diff(idx_a) > 0).all()   # seeded, in line order
    boxes = np.concatenate([p["boxes"] for p in lib.h[0]])
    assert np.array_equal(np.load(tmp_path / "a" / "boxes.npy"), boxes[idx_a.astype(np.int64)])

"""Directory batch driver: the retto-cli loop (/root/reference/retto-cli/src/main.rs:41-95) over the
HIP session -- walk a directory, decode every file on the host (like the reference's
ImageHelper::new_from_raw_img_flow), run the pages through RettoSession in batches, log the
average time per image.  Model files are RTWB blobs (retto_amd/synth.py; converting the PP-OCRv4
.onnx files is SURVEY 8(f) rank 1); ``--synthetic`` uses seeded synthetic weights.

    python -m retto_amd.cli --images DIR [--batch 32] [--device-id 0] [--json OUT.jsonl]
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import time

import numpy as np

log = logging.getLogger("retto_cli")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="retto-cli (hip)")
    ap.add_argument("--det-model-path", default="ch_PP-OCRv4_det_infer.rtwb")
    ap.add_argument("--cls-model-path", default="ch_ppocr_mobile_v2.0_cls_infer.rtwb")
    ap.add_argument("--rec-model-path", default="ch_PP-OCRv4_rec_infer.rtwb")
    ap.add_argument("--rec-keys-path", default="ppocr_keys_v1.txt")
    ap.add_argument("-i", "--images", required=True)
    ap.add_argument("--device", choices=["hip"], default="hip", help="only the MI355X HIP backend exists here")
    ap.add_argument("--device-id", type=int, default=0)
    ap.add_argument("--batch", type=int, default=32, help="pages per rt_run_batch call")
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights + dictionary instead of model files")
    ap.add_argument("--json", default=None, help="write one JSON object per image (det/cls/rec stage results)")
    ap.add_argument("--det-score-mode", choices=["Fast", "Slow"], default="Fast",
                    help="DetProcessorConfig.score_mode: box score over the min-area rect (Fast) or the contour's own polygon (Slow)")
    ap.add_argument("--rec-return-word-box", action="store_true",
                    help="RecProcessorConfig.return_word_box: per-word boxes; each --json line gains a \"words\" array (per line)")
    ap.add_argument("--rec-candidates", type=int, default=0, metavar="K",
                    help="RecProcessorConfig.return_candidates: K = 1..8 candidates per token; each --json line gains "
                         "\"candidates\" and \"token_cols\" arrays (per line)")
    ap.add_argument("--crop-source", choices=["Resized", "Original"], default="Resized",
                    help="RettoSessionConfig.crop_source: cut the text lines from the page after resize_both (Resized, the "
                         "reference) or from the page as it was read (Original: small print on pages above max_side_len)")
    ap.add_argument("--rec-charset", default=None, metavar="TEXT",
                    help="restrict every line's CTC decode to these characters (one charset, made the session default): the "
                         "dictionary classes whose whole entry is one character of TEXT, plus the blank")
    ap.add_argument("--rec-lexicon", default=None, metavar="FILE",
                    help="a word list, one entry per line: every line's result also ranks these entries by their CTC forward "
                         "log-likelihood (one lexicon, made the session default; the recognised text itself is unchanged unless --rec-lexicon-snap is given)")
    ap.add_argument("--rec-pattern", default=None, metavar="TEXT",
                    help="constrain every line's text to this regular expression over the dictionary, e.g. "
                         "'[0-9]{4}-[0-9]{2}-[0-9]{2}' (one pattern, made the session default; not together with --rec-lexicon)")
    ap.add_argument("--rec-lexicon-snap", type=float, default=None, metavar="P",
                    help="with --rec-lexicon: a line whose best entry's posterior reaches P (0 < P <= 1) takes that entry, "
                         "aligned to its time steps, as its text, score, words and candidates (\"lexicon_snapped\" per line)")
    ap.add_argument("--det-tile", type=int, default=0, metavar="N",
                    help="detect pages whose det input is larger than N pixels either way as overlapping N x N tiles, stitched "
                         "into one page map (large scans at their own resolution); a multiple of 32, at least 64; 0 = off")
    ap.add_argument("--det-tile-overlap", type=int, default=64, metavar="M",
                    help="with --det-tile: the tiles' overlap, a multiple of 32, at most N / 2")
    ap.add_argument("--rec-window", type=int, default=0, metavar="N",
                    help="read rec lines at least 8 columns wider than N as overlapping windows of N columns, stitched into the "
                         "one line (long lines at a familiar width; the effect on accuracy is not measured); a multiple of 32, "
                         "at least 128; 0 = off")
    ap.add_argument("--rec-window-overlap", type=int, default=0, metavar="M",
                    help="with --rec-window: the windows' overlap, a multiple of 32, at most N / 2")
    ap.add_argument("--rec-beam", default=None, metavar="B[,N]",
                    help="rec beams: every line also reports its N (default 1) most probable strings from a CTC prefix beam "
                         "search of width B (1..32; N up to min(B, 8)); each --json line gains a \"beams\" array (per line)")
    ap.add_argument("--rec-lm", default=None, metavar="FILE",
                    help="with --rec-beam: a character n-gram language model in ARPA text over the dictionary (tokens: one "
                         "dictionary entry each, <sp> the space, <s> the line start), fused into the beam search; the "
                         "hypotheses gain \"lm_logprob\" and \"lm_score\" (the effect on accuracy is not measured)")
    ap.add_argument("--rec-lm-weights", default="1.0,0.0", metavar="ALPHA,BETA",
                    help="with --rec-lm: the beam keeps the candidates with the best logprob + ALPHA * lm + BETA * length")
    ap.add_argument("--rec-vocab", default=None, metavar="FILE",
                    help="with --rec-beam: a word list, one word per line in UTF-8 over the dictionary, fused into the beam search: "
                         "every word of a hypothesis that is not in the list costs G; characters the list does not spell with "
                         "(digits, punctuation, the space) pass freely and separate words; the hypotheses gain \"oov_words\" and "
                         "\"vocab_score\" (the effect on accuracy is not measured)")
    ap.add_argument("--rec-vocab-gamma", type=float, default=4.0, metavar="G",
                    help="with --rec-vocab: the cost of a word that is not in the list, in nats (default 4.0)")
    ap.add_argument("--rec-vocab-case-variants", action="store_true",
                    help="with --rec-vocab: every word also Capitalised and in UPPER CASE")
    ap.add_argument("--rec-flip", type=float, default=0.0, metavar="CLS_BELOW",
                    help="read lines whose classifier score is below CLS_BELOW both ways up and keep the reading with the better "
                         "greedy CTC score (such a line costs the rec network twice; the effect on accuracy is not measured); "
                         "above 1 = every line; 0 = off")
    return ap


def parse_beam(text: str):
    """--rec-beam's "B" or "B,N" -> (B, N)"""
    parts = text.split(",")
    if len(parts) not in (1, 2) or not all(p.strip().lstrip("+").isdigit() for p in parts):
        raise SystemExit("--rec-beam takes B or B,N")
    return int(parts[0]), int(parts[1]) if len(parts) == 2 else 1


def parse_weights(text: str):
    """--rec-lm-weights' "ALPHA,BETA" -> (alpha, beta)"""
    try:
        alpha, beta = (float(p) for p in text.split(","))
    except ValueError:
        raise SystemExit("--rec-lm-weights takes ALPHA,BETA")
    return alpha, beta


def walk_files(root: str):
    """WalkDir semantics of main.rs:72-77: every regular file under root, directory order."""
    out = []
    for d, dirs, files in os.walk(root):
        dirs.sort()
        for f in sorted(files):
            out.append(os.path.join(d, f))
    return out


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s %(name)s: %(message)s")
    import retto_amd
    if a.synthetic:
        cfg = retto_amd.synthetic_session_config(0, device=a.device_id)
    else:
        cfg = retto_amd.RettoSessionConfig()
        S = retto_amd.RettoWorkerModelSource
        cfg.worker_config = retto_amd.RettoHipWorkerConfig(device=a.device_id, models=retto_amd.RettoWorkerModelProvider(
            det=S.Path(a.det_model_path), rec=S.Path(a.rec_model_path), cls=S.Path(a.cls_model_path)))
        cfg.rec_processor_config.character_source = S.Path(a.rec_keys_path)
    cfg.det_processor_config.score_mode = a.det_score_mode
    cfg.rec_processor_config.return_word_box = a.rec_return_word_box
    cfg.rec_processor_config.return_candidates = a.rec_candidates
    cfg.crop_source = a.crop_source
    session = retto_amd.RettoSession(cfg)
    if a.det_tile:
        session.set_det_tiles(a.det_tile, a.det_tile_overlap)
    if a.rec_window:
        session.set_rec_windows(a.rec_window, a.rec_window_overlap)
    if a.rec_flip:
        session.set_rec_flip(a.rec_flip)
    if a.rec_charset is not None:
        session.set_rec_charset(session.create_charset(a.rec_charset))
    if a.rec_lexicon is not None:
        with open(a.rec_lexicon, "rb") as f:
            lexicon = session.create_lexicon(f.read())
        if a.rec_lexicon_snap is not None:
            session.set_lexicon_snap(lexicon, a.rec_lexicon_snap)
        session.set_rec_lexicon(lexicon)
    elif a.rec_lexicon_snap is not None:
        raise SystemExit("--rec-lexicon-snap needs --rec-lexicon")
    if a.rec_pattern is not None:
        if a.rec_lexicon is not None:
            raise SystemExit("--rec-pattern and --rec-lexicon exclude each other")
        session.set_rec_pattern(session.create_pattern(a.rec_pattern))
    if a.rec_beam is not None:
        session.set_rec_beam(*parse_beam(a.rec_beam))
    if a.rec_lm is not None:
        if a.rec_beam is None:
            raise SystemExit("--rec-lm needs --rec-beam")
        with open(a.rec_lm, "rb") as f:
            session.set_rec_beam_lm(session.create_lm(f.read()), *parse_weights(a.rec_lm_weights))
    if a.rec_vocab is not None:
        if a.rec_beam is None:
            raise SystemExit("--rec-vocab needs --rec-beam")
        with open(a.rec_vocab, "rb") as f:
            session.set_rec_beam_vocab(session.create_vocab(f.read(), case_variants=a.rec_vocab_case_variants), a.rec_vocab_gamma)
    files = walk_files(a.images)
    log.info("Found %d files, processing...", len(files))
    out = open(a.json, "w") if a.json else None
    start = time.perf_counter()
    n = 0
    for s0 in range(0, len(files), a.batch):
        chunk = files[s0:s0 + a.batch]
        pages = []
        for path in chunk:
            with open(path, "rb") as fh:
                pages.append(retto_amd.decode_image(fh.read()))  # a decode failure aborts, like expect() in main.rs:83
        results = session.run_batch(pages)
        n += len(results)
        if out:
            for path, r in zip(chunk, results):
                rec = {
                    "file": path,
                    "det": [{"boxes": {"inner": [{"x": p.x, "y": p.y} for p in d.boxes.inner]}, "score": d.score} for d in r.det_result],
                    "cls": [{"label": {"label": c.label.label, "score": c.label.score}} for c in r.cls_result],
                    "rec": [{"text": t.text, "score": None if np.isnan(t.score) else t.score} for t in r.rec_result],
                }
                if a.rec_return_word_box:   # one list of words per line, in line order
                    rec["words"] = [[{"text": w.text, "kind": w.kind, "boxes": {"inner": [{"x": p.x, "y": p.y} for p in w.box.inner]},
                                      "first_token": w.first_token, "n_tokens": w.n_tokens, "first_col": w.first_col,
                                      "last_col": w.last_col} for w in t.words] for t in r.rec_result]
                if a.rec_candidates:   # per line: one list of K {id, text, prob} per token, and the tokens' time steps
                    rec["candidates"] = [[[{"id": i, "text": s, "prob": p} for i, s, p in tok] for tok in t.candidates]
                                         for t in r.rec_result]
                    rec["token_cols"] = [[int(c) for c in t.token_cols] for t in r.rec_result]
                if a.rec_lexicon is not None:   # per line: up to 4 {entry, text, loglik, posterior}, best first
                    rec["lexicon_matches"] = [[{"entry": e, "text": s, "loglik": ll, "posterior": p}
                                               for e, s, ll, p in (t.lexicon_matches or [])] for t in r.rec_result]
                    if a.rec_lexicon_snap is not None:   # per line: whether its text is its aligned best entry
                        rec["lexicon_snapped"] = [bool(t.lexicon_snapped) for t in r.rec_result]
                if a.rec_pattern is not None:   # per line: {matched, logprob, free_logprob} (logprob null where unmatched)
                    rec["pattern"] = [None if t.pattern is None else
                                      {"matched": t.pattern[0], "logprob": t.pattern[1] if t.pattern[0] else None,
                                       "free_logprob": t.pattern[2]} for t in r.rec_result]
                if a.rec_beam is not None:   # per line: its hypotheses, best first; lm_logprob / lm_score with --rec-lm
                    rec["beams"] = [[dict({"text": h.text, "tokens": [int(c) for c in h.tokens], "logprob": h.logprob},
                                          **({} if h.lm_score is None else {"lm_logprob": h.lm_logprob, "lm_score": h.lm_score}),
                                          **({} if h.vocab_score is None else {"oov_words": h.oov_words, "vocab_score": h.vocab_score}))
                                     for h in (t.beams or [])] for t in r.rec_result]
                out.write(json.dumps(rec, ensure_ascii=False) + "\n")
    dur = time.perf_counter() - start
    if out:
        out.close()
    if n:
        log.info("Successfully processed %d images, avg time: %.2fms", n, 1000.0 * dur / n)
    session.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""retto_amd -- Python host-side mirror of retto-core's worker / session interface on
top of libretto_hip.so (MI355X / gfx950).

Names follow the reference (paths relative to /root/reference/retto-core/src):
    RettoWorkerModelSource  worker.rs:18-27        RettoHipWorker        worker.rs:69-98 (+ ort_worker.rs)
    RettoSessionConfig      session.rs:17-40       RettoSession.run      session.rs:108-131
    RettoWorkerResult       session.rs:44-48       RettoSession.run_stream  session.rs:133-143
    Point / PointBox        points.rs:16-68        Det/Cls/RecProcessorResult  processor/*.rs
Everything is computed by the HIP library; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import io
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import Config, ModelSource, RT_MEM_DEVICE, RT_MEM_HOST, RT_MEM_HOST_MAPS_DEVICE, RT_MAX_INFLIGHT


# ---- errors (error.rs:2-21) ------------------------------------------------------------
class RettoError(Exception):
    code = 4


class IOError_(RettoError): code = 1
class ImageError(RettoError): code = 2
class ShapeError(RettoError): code = 3
class BackendError(RettoError): code = 4
class Utf8Error(RettoError): code = 5
class ModelNotFoundError(RettoError): code = 7
class InvalidArgument(RettoError): code = 8
class CapacityError(RettoError): code = 9


_ERRS = {c.code: c for c in (IOError_, ImageError, ShapeError, BackendError, Utf8Error, ModelNotFoundError,
                             InvalidArgument, CapacityError)}


def _check(rc: int, handle) -> None:
    if rc != 0:
        msg = _lib.load().rt_last_error(handle)
        raise _ERRS.get(rc, RettoError)((msg or b"").decode("utf-8", "replace"))


# ---- model sources (worker.rs:18-27) -----------------------------------------------------
@dataclass
class RettoWorkerModelSource:
    path: Optional[str] = None
    blob: Optional[bytes] = None

    @staticmethod
    def Path(p: str) -> "RettoWorkerModelSource":
        return RettoWorkerModelSource(path=p)

    @staticmethod
    def Blob(b: bytes) -> "RettoWorkerModelSource":
        return RettoWorkerModelSource(blob=bytes(b))


@dataclass
class RettoWorkerModelProvider:  # worker.rs:61-65
    det: RettoWorkerModelSource
    rec: RettoWorkerModelSource
    cls: RettoWorkerModelSource


@dataclass
class RettoHipWorkerConfig:  # RettoOrtWorkerConfig analogue (ort_worker.rs:53-56)
    device: int = 0
    models: Optional[RettoWorkerModelProvider] = None


@dataclass
class DetProcessorConfig:  # det_processor.rs:44-93
    limit_side_len: int = 736
    limit_type: str = "Min"
    mean: Sequence[float] = (0.5, 0.5, 0.5)
    std: Sequence[float] = (0.5, 0.5, 0.5)
    scale: float = float(np.float32(1.0) / np.float32(255.0))
    threch: float = 0.3
    box_thresh: float = 0.5
    max_candidates: int = 1000  # declared but never read by the reference either
    unclip_ratio: float = 1.6
    use_dilation: bool = True
    min_mini_box_size: int = 3
    dilation_kernel: Optional[np.ndarray] = field(default_factory=lambda: np.ones((2, 2), np.uint64))
    score_mode: str = "Fast"  # ScoreMode (det_processor.rs:22-31): "Fast" = min-area rect, "Slow" = the contour's own polygon


@dataclass
class ClsProcessorConfig:  # cls_processor.rs:14-36
    image_shape: Sequence[int] = (3, 48, 192)
    batch_num: int = 6
    thresh: float = 0.9
    label: Sequence[int] = (0, 180)


@dataclass
class RecProcessorConfig:  # rec_processor.rs:102-136
    character_source: Optional[RettoWorkerModelSource] = None
    image_shape: Sequence[int] = (3, 48, 320)
    batch_num: int = 6
    # RecCharacter::decode's return_word_box (rec_processor.rs:48-56; the reference never implements it): per-word boxes in
    # RecProcessorSingleResult.words (include/retto_hip.h "word boxes" for the rule)
    return_word_box: bool = False
    # rt_config.rec_return_candidates: 0 = off, K = 1..8: per kept token its time step (RecProcessorSingleResult.token_cols) and K
    # candidates (.candidates): the token itself, then the K - 1 next best classes (include/retto_hip.h "token candidates")
    return_candidates: int = 0


@dataclass
class RettoSessionConfig:  # session.rs:17-40
    worker_config: RettoHipWorkerConfig = field(default_factory=RettoHipWorkerConfig)
    max_side_len: int = 2000
    min_side_len: int = 30
    det_processor_config: DetProcessorConfig = field(default_factory=DetProcessorConfig)
    cls_processor_config: ClsProcessorConfig = field(default_factory=ClsProcessorConfig)
    rec_processor_config: RecProcessorConfig = field(default_factory=RecProcessorConfig)
    max_boxes_per_page: int = 0
    det_sub_batch: int = 0
    lanes: int = 0
    dtype: str = "f32"   # "f32" (the reference's arithmetic) or "f16" (fp16 storage / MFMA, fp32 accumulation)
    # rt_config.crop_source: "Resized" (the reference: lines are cut from the page after resize_both) or "Original" (from the page
    # as handed in, by the boxes the results report; include/retto_hip.h states the rule)
    crop_source: str = "Resized"


# ---- result types (points.rs, processor/*.rs) ---------------------------------------------
@dataclass
class Point:
    x: float
    y: float


@dataclass
class PointBox:
    inner: List[Point]  # clockwise from top-left

    def tl(self): return self.inner[0]
    def tr(self): return self.inner[1]
    def br(self): return self.inner[2]
    def bl(self): return self.inner[3]

    def as_array(self) -> np.ndarray:
        return np.array([[p.x, p.y] for p in self.inner], np.float32)


@dataclass
class DetProcessorInnerResult:
    boxes: PointBox
    score: float


@dataclass
class ClsPostProcessLabel:
    label: int
    score: float


@dataclass
class ClsProcessorSingleResult:
    label: ClsPostProcessLabel


@dataclass
class RecWord:
    """One word of a line (rt_word): its text, its quad in original-image coordinates, kind "cjk" (one CJK character) or
    "alnum" (a run of ASCII letters / digits with inner "." / "-"), its kept-token range and first / last time step."""
    text: str
    box: PointBox
    kind: str
    first_token: int
    n_tokens: int
    first_col: int
    last_col: int


@dataclass
class KeywordHit:   # rt_keyword_hit, with the entry's text
    entry: int
    text: str
    score: float          # log-ratio of the best path that contains the entry to the best path; <= 0, 0: the greedy path holds it
    first_col: int
    last_col: int
    box: np.ndarray       # [4, 2] the span's page quad, TL, TR, BR, BL in original-image coordinates


@dataclass
class BeamHypothesis:   # rt_beam, with its tokens and text
    tokens: np.ndarray    # int32 class ids in reading order; empty: the empty string
    text: str
    logprob: float        # log of the summed probability of the string's alignments that stayed inside the beam
    # rec language model (set_rec_beam_lm; rt_beam_lm): None when fusion was off, else the model's sum over the string (natural
    # log) and the fused score logprob + (alpha * lm_logprob + beta * len(tokens)) the hypotheses are ordered by
    lm_logprob: Optional[float] = None
    lm_score: Optional[float] = None
    # rec vocabulary (set_rec_beam_vocab; rt_beam_vocab): None when no vocabulary was attached, else the string's words that are
    # not in the list (the line end closing the last one) and the score -- logprob, or lm_score with a model, minus gamma per
    # such word -- the hypotheses are ordered by
    oov_words: Optional[int] = None
    vocab_score: Optional[float] = None


@dataclass
class RecFlip:   # rt_results_rec_flip
    outcome: int     # 1: the line was read both ways up and view 0 (the crop as the classifier left it) was kept; 2: view 1 taken
    score0: float    # the views' greedy CTC scores; NaN for a view that kept no token
    score1: float


@dataclass
class RecProcessorSingleResult:
    text: str
    score: float
    tokens: np.ndarray = None  # kept CTC token ids (not in the reference struct; exposed for parity checks)
    words: Optional[List[RecWord]] = None  # RecProcessorConfig.return_word_box; None when off
    # RecProcessorConfig.return_candidates = K; None when off.  candidates: per kept token a list of K (id, text, prob), rank 0 the
    # token itself with the probability the score averages, then the next best classes (id -1, text "" where the model has fewer
    # than K classes); token_cols: the tokens' time steps
    candidates: Optional[List[List[Tuple[int, str, float]]]] = None
    token_cols: Optional[np.ndarray] = None
    # rec lexicons (create_lexicon): None when the line carried no lexicon, else up to LEXICON_MATCHES (entry, text, loglik,
    # posterior), best first: the lexicon's entries ranked by their CTC forward log-likelihood under the line's own distribution
    lexicon_matches: Optional[List[Tuple[int, str, float, float]]] = None
    # lexicon snap (set_lexicon_snap): None when the line carried no lexicon, else whether the line's text, tokens, score, words
    # and candidates are those of its best entry (lexicon_matches[0]) aligned to the line, instead of the greedy decode
    lexicon_snapped: Optional[bool] = None
    # rec patterns (create_pattern): None when the line carried no pattern, else (matched, logprob, free_logprob): whether the
    # line's decode is the best CTC path the pattern accepts, that path's log-probability (-inf where unmatched) and the
    # unconstrained best path's; logprob - free_logprob <= 0 is what the format cost
    pattern: Optional[Tuple[bool, float, float]] = None
    # rec keywords (create_keywords): None when the line carried no list, else up to KEYWORD_HITS hits, best first: the list's
    # entries spotted inside the line (retto_amd/csrc/ctc_keyword.h)
    keywords: Optional[List["KeywordHit"]] = None
    # rec beams (set_rec_beam): None when the option is off, else the line's most probable strings by CTC prefix beam search,
    # best first (retto_amd/csrc/ctc_beam.h)
    beams: Optional[List["BeamHypothesis"]] = None
    # rec windows (set_rec_windows): the number of units the line was read in, 1 for a whole line (retto_amd/csrc/rec_windows.h)
    windows: int = 1
    # rec flip (set_rec_flip): None when the line was read one way, else the outcome and the two views' scores
    # (retto_amd/csrc/rec_flip.h)
    flip: Optional["RecFlip"] = None


@dataclass
class RettoWorkerResult:  # session.rs:44-48
    det_result: List[DetProcessorInnerResult]
    cls_result: List[ClsProcessorSingleResult]
    rec_result: List[RecProcessorSingleResult]


def _src(s: Optional[RettoWorkerModelSource], keep: list) -> ModelSource:
    m = ModelSource()
    if s is None:
        return m
    if s.path is not None:
        b = s.path.encode("utf-8"); keep.append(b); m.path = b
    elif s.blob is not None:
        buf = C.create_string_buffer(s.blob, len(s.blob)); keep.append(buf)
        m.data = C.cast(buf, C.c_void_p); m.len = len(s.blob)
    return m


def _as_f32(a, ndim):
    a = np.ascontiguousarray(a, np.float32)  # as_standard_layout (ort_worker.rs:191,202,213)
    if a.ndim != ndim:
        raise ShapeError(f"expected {ndim}-d array, got {a.ndim}-d")
    return a


class _Handle:
    """Owns one rt_session (one GPU)."""

    def __init__(self, cfg: RettoSessionConfig):
        lib = _lib.load()
        c = Config()
        lib.rt_config_default(C.byref(c))
        keep: list = []
        wc = cfg.worker_config
        if wc.models is None:
            raise ModelNotFoundError("no model provider configured (worker_config.models)")
        c.device_id = wc.device
        c.det = _src(wc.models.det, keep); c.cls = _src(wc.models.cls, keep); c.rec = _src(wc.models.rec, keep)
        c.dict = _src(cfg.rec_processor_config.character_source, keep)
        c.max_side_len, c.min_side_len = cfg.max_side_len, cfg.min_side_len
        d = cfg.det_processor_config
        c.det_limit_side_len = d.limit_side_len
        c.det_limit_type = 0 if d.limit_type == "Min" else 1
        for i in range(3):
            c.det_mean[i] = d.mean[i]; c.det_std[i] = d.std[i]
        c.det_scale = d.scale; c.det_thresh = d.threch; c.det_box_thresh = d.box_thresh
        c.det_unclip_ratio = d.unclip_ratio; c.det_min_mini_box_size = d.min_mini_box_size
        if d.dilation_kernel is None:
            c.det_dilation = 0
        else:
            k = np.asarray(d.dilation_kernel)
            if k.shape != (2, 2) or not np.all(k != 0):
                raise InvalidArgument("only the reference's default 2x2 all-ones dilation kernel (or None) is supported")
            c.det_dilation = 1
        if d.score_mode not in ("Fast", "Slow"):
            raise InvalidArgument("score_mode must be 'Fast' or 'Slow'")
        c.det_score_mode = 1 if d.score_mode == "Slow" else 0
        cl, rc = cfg.cls_processor_config, cfg.rec_processor_config
        for i in range(3):
            c.cls_image_shape[i] = cl.image_shape[i]; c.rec_image_shape[i] = rc.image_shape[i]
        c.cls_batch_num, c.cls_thresh = cl.batch_num, cl.thresh
        c.rec_batch_num = rc.batch_num
        c.rec_return_word_box = 1 if rc.return_word_box else 0
        c.rec_return_candidates = int(rc.return_candidates)
        if tuple(cl.label) != (0, 180):
            raise InvalidArgument("cls label set other than [0, 180] is not supported")
        c.max_boxes_per_page = cfg.max_boxes_per_page; c.det_sub_batch = cfg.det_sub_batch; c.lanes = cfg.lanes
        if cfg.dtype not in ("f32", "f16"):
            raise InvalidArgument("dtype must be 'f32' or 'f16'")
        c.dtype = 1 if cfg.dtype == "f16" else 0
        if cfg.crop_source not in ("Resized", "Original"):
            raise InvalidArgument("crop_source must be 'Resized' or 'Original'")
        c.crop_source = 1 if cfg.crop_source == "Original" else 0
        h = C.c_void_p()
        _check(lib.rt_create(C.byref(c), C.byref(h)), None)
        self.lib, self.h = lib, h

    def close(self):
        if getattr(self, "h", None):
            self.lib.rt_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RettoHipWorker:
    """``impl RettoWorker + RettoInnerWorker`` for the HIP backend (worker.rs:69-98)."""

    def __init__(self, cfg: Union[RettoSessionConfig, RettoHipWorkerConfig], _handle: Optional[_Handle] = None):
        if _handle is None:
            if isinstance(cfg, RettoHipWorkerConfig):
                raise InvalidArgument("construct RettoHipWorker from a RettoSessionConfig (the dictionary is needed)")
            _handle = _Handle(cfg)
        self._hd = _handle

    def init(self) -> None:  # worker.rs:97 (no-op like ort_worker.rs:183-185)
        return None

    def det(self, x: np.ndarray) -> np.ndarray:
        x = _as_f32(x, 4); n, c, h, w = x.shape
        out = np.empty((n, 1, h, w), np.float32)
        _check(self._hd.lib.rt_det(self._hd.h, x.ctypes.data, n, c, h, w, out.ctypes.data), self._hd.h)
        return out

    def cls(self, x: np.ndarray) -> np.ndarray:
        x = _as_f32(x, 4); n, c, h, w = x.shape
        out = np.empty((n, 2), np.float32)
        _check(self._hd.lib.rt_cls(self._hd.h, x.ctypes.data, n, c, h, w, out.ctypes.data), self._hd.h)
        return out

    def rec(self, x: np.ndarray) -> np.ndarray:
        x = _as_f32(x, 4); n, c, h, w = x.shape
        t = C.c_int()
        _check(self._hd.lib.rt_rec(self._hd.h, x.ctypes.data, n, c, h, w, None, C.byref(t)), self._hd.h)
        out = np.empty((n, t.value, self._hd.lib.rt_rec_classes(self._hd.h)), np.float32)
        _check(self._hd.lib.rt_rec(self._hd.h, x.ctypes.data, n, c, h, w, out.ctypes.data, C.byref(t)), self._hd.h)
        return out


    def rec_ragged(self, lines) -> list:
        """rt_rec_ragged: lines = [3,48,w_i] arrays of different widths, ONE launch series (the form rt_run_batch's rec groups
        take); returns the per-line [T_i, classes] probabilities."""
        lines = [_as_f32(l, 3) for l in lines]
        n = len(lines)
        widths = (C.c_int * n)(*[l.shape[2] for l in lines])
        ts = (C.c_int * n)()
        flat = np.ascontiguousarray(np.concatenate([l.reshape(-1) for l in lines]))
        _check(self._hd.lib.rt_rec_ragged(self._hd.h, flat.ctypes.data, n, widths, None, ts), self._hd.h)
        ncls = self._hd.lib.rt_rec_classes(self._hd.h)
        out = np.empty((sum(ts), ncls), np.float32)
        _check(self._hd.lib.rt_rec_ragged(self._hd.h, flat.ctypes.data, n, widths, out.ctypes.data, ts), self._hd.h)
        res, o = [], 0
        for t in ts:
            res.append(out[o:o + t]); o += t
        return res

def decode_image(data: bytes) -> np.ndarray:
    """ImageHelper::new_from_raw_img_flow (image_helper.rs:34-44): encoded bytes -> RGB8 [H,W,3] through the
    library's host decoder (rt_decode_image: PNG, JPEG, PNM, BMP); raises ImageError otherwise."""
    lib = _lib.load()
    data = bytes(data)
    out = C.c_void_p(); h = C.c_int(); w = C.c_int()
    err = C.create_string_buffer(512)
    rc = lib.rt_decode_image(data, len(data), C.byref(out), C.byref(h), C.byref(w), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)(err.value.decode("utf-8", "replace"))
    try:
        return np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (h.value, w.value, 3)).copy()
    finally:
        lib.rt_buffer_free(out)


def debug_jpeg_reconstruct(data: bytes):
    """rt_debug_jpeg_reconstruct: the device decode path's host stage plus the reconstruction kernels' arithmetic, run on the
    CPU.  Returns (RGB8 [H,W,3], on_device); on_device False means the device path decodes this file on the host."""
    lib = _lib.load()
    data = bytes(data)
    out = C.c_void_p(); h = C.c_int(); w = C.c_int(); dev = C.c_int()
    err = C.create_string_buffer(512)
    rc = lib.rt_debug_jpeg_reconstruct(data, len(data), C.byref(out), C.byref(h), C.byref(w), C.byref(dev), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)(err.value.decode("utf-8", "replace"))
    try:
        return np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (h.value, w.value, 3)).copy(), bool(dev.value)
    finally:
        lib.rt_buffer_free(out)


def _rec_word(w, text: str) -> RecWord:
    q = [float(v) for v in w.quad]
    return RecWord(text, PointBox([Point(q[2 * i], q[2 * i + 1]) for i in range(4)]), "cjk" if w.kind == 0 else "alnum",
                   int(w.first_token), int(w.n_tokens), int(w.first_col), int(w.last_col))


def debug_word_boxes(dict_bytes: bytes, tokens, cols, T: int, W: int, resized_w: int, box_after, rot180: bool,
                     after_w: int, after_h: int, ori_w: int, ori_h: int) -> List[RecWord]:
    """rt_debug_word_boxes: the word rule (retto_amd/csrc/word_boxes.h) on the CPU for one line.  tokens / cols: kept class
    ids and their time steps; box_after: the line's det box [4,2] in after-resize_both coordinates.  Word texts are the
    dictionary entries of each word's tokens."""
    lib = _lib.load()
    dict_bytes = bytes(dict_bytes)
    tok = np.ascontiguousarray(tokens, np.int32); col = np.ascontiguousarray(cols, np.int32)
    n = len(tok)
    if len(col) != n:
        raise ShapeError("tokens and cols differ in length")
    box = np.ascontiguousarray(box_after, np.float32).reshape(8)
    out = (_lib.Word * max(n, 1))(); nw = C.c_int()
    P = C.POINTER
    rc = lib.rt_debug_word_boxes(dict_bytes, len(dict_bytes), tok.ctypes.data_as(P(C.c_int32)), col.ctypes.data_as(P(C.c_int32)),
                                 n, T, W, resized_w, box.ctypes.data_as(P(C.c_float)), 1 if rot180 else 0, after_w, after_h,
                                 ori_w, ori_h, out, C.byref(nw))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)("rt_debug_word_boxes failed")
    ents = parse_dictionary(dict_bytes)
    return [_rec_word(out[j], "".join(ents[int(t)] for t in tok[out[j].first_token:out[j].first_token + out[j].n_tokens]))
            for j in range(nw.value)]


def _candidate_lists(cands, K: int, n_tokens: int, entries: Sequence[str]) -> List[List[Tuple[int, str, float]]]:
    """rt_candidate [n_tokens][K] -> per token its K (id, text, prob); text from the dictionary entries, "" for the fill id -1."""
    return [[(int(c.id), entries[c.id] if c.id >= 0 else "", float(c.prob)) for c in (cands[j * K + q] for q in range(K))]
            for j in range(n_tokens)]


def debug_charset_compile(dict_bytes: bytes, text: str = "", ids: Sequence[int] = ()) -> np.ndarray:
    """rt_debug_charset_compile: what RettoSession.create_charset compiles (retto_amd/csrc/ctc_charset.h), GPU-free: the mask
    of the charset as uint32 words, class c at bit (c & 31) of word c >> 5.  text: str, or bytes to pass raw UTF-8."""
    lib = _lib.load()
    dict_bytes = bytes(dict_bytes)
    raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    arr = (C.c_int32 * max(len(ids), 1))(*[int(i) for i in ids])
    n = C.c_int(); err = C.create_string_buffer(256)
    lib.rt_debug_charset_compile(dict_bytes, len(dict_bytes), raw, len(raw), arr, len(ids), None, 0, C.byref(n), err, len(err))
    mask = np.zeros(max((n.value + 31) // 32, 1), np.uint32)
    rc = lib.rt_debug_charset_compile(dict_bytes, len(dict_bytes), raw, len(raw), arr, len(ids), mask.ctypes.data, len(mask),
                                      C.byref(n), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)(err.value.decode("utf-8", "replace"))
    return mask


def _lexicon_id_arrays(ids):
    """entries given as class ids -> (flat ids, lengths, count) as ctypes arrays"""
    ids = [[int(c) for c in e] for e in ids]
    flat = [c for e in ids for c in e]
    return (C.c_int32 * max(len(flat), 1))(*flat), (C.c_int32 * max(len(ids), 1))(*[len(e) for e in ids]), len(ids)


def _lexicon_text(entries) -> bytes:
    return entries if isinstance(entries, (bytes, bytearray)) else "\n".join(entries).encode("utf-8")


def debug_lexicon_compile(dict_bytes: bytes, entries=(), ids=()) -> List[List[int]]:
    """rt_debug_lexicon_compile: what RettoSession.create_lexicon compiles (retto_amd/csrc/ctc_lexicon.h), GPU-free: every
    entry as its list of class ids.  entries: strings (one entry each), or bytes to pass raw UTF-8 lines; ids: entries given as
    class ids, appended."""
    lib = _lib.load()
    dict_bytes = bytes(dict_bytes)
    raw = bytes(_lexicon_text(entries))
    arr, lens, n_id = _lexicon_id_arrays(ids)
    ni, ne, nc = C.c_int(), C.c_int(), C.c_int()
    err = C.create_string_buffer(256)
    cap_i, cap_e = len(raw) + len(arr) + 1, raw.count(b"\n") + n_id + 2
    out_i = np.zeros(cap_i, np.int32); out_e = np.zeros(cap_e, np.int32)
    rc = lib.rt_debug_lexicon_compile(dict_bytes, len(dict_bytes), raw, len(raw), arr, lens, n_id, out_i.ctypes.data, cap_i,
                                      out_e.ctypes.data, cap_e, C.byref(ni), C.byref(ne), C.byref(nc), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)(err.value.decode("utf-8", "replace"))
    offs = np.concatenate([[0], np.cumsum(out_e[:ne.value])])
    return [out_i[offs[j]:offs[j + 1]].tolist() for j in range(ne.value)]


def debug_pattern_compile(dict_bytes: bytes, pattern) -> dict:
    """rt_debug_pattern_compile: a rec pattern's compiled form (retto_amd/csrc/ctc_pattern.h), GPU-free: a dict with
    group_of [classes], delta [S][G] (-1: no arc), accept [S] as int32 arrays and S, G, P, min_steps, classes.  pattern: a
    string, or bytes to pass raw UTF-8."""
    lib = _lib.load()
    dict_bytes = bytes(dict_bytes)
    raw = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
    S, G, P, ms, nc = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    err = C.create_string_buffer(384)
    cap_g = dict_bytes.count(b"\n") + 3
    group_of = np.zeros(cap_g, np.int32); delta = np.zeros(_lib.PATTERN_MAX_STATES * cap_g, np.int32)
    accept = np.zeros(_lib.PATTERN_MAX_STATES, np.int32)
    rc = lib.rt_debug_pattern_compile(dict_bytes, len(dict_bytes), raw, len(raw), group_of.ctypes.data, len(group_of),
                                      delta.ctypes.data, len(delta), accept.ctypes.data, len(accept), C.byref(S), C.byref(G),
                                      C.byref(P), C.byref(ms), C.byref(nc), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)(err.value.decode("utf-8", "replace"))
    return {"group_of": group_of[:nc.value].copy(), "delta": delta[:S.value * G.value].reshape(S.value, G.value).copy(),
            "accept": accept[:S.value].copy(), "S": S.value, "G": G.value, "P": P.value, "min_steps": ms.value,
            "classes": nc.value}


_TILE_PLAN_BUFS = None   # the four output arrays of det_tile_plan, grown on demand (a plan grid asks a hundred thousand times)


def det_tile_plan(h: int, w: int, tile: int, overlap: int = 64) -> dict:
    """rt_det_tile_plan: the det tile plan (retto_amd/csrc/det_tiles.h) of a det input of h x w, GPU-free: a dict with tile_h,
    tile_w, and per direction the tiles' origins and ownership bounds (tile i owns [bounds[i - 1], bounds[i]), from 0) as
    lists: row_origins, row_bounds, col_origins, col_bounds.  Tiles are in row-major order."""
    global _TILE_PLAN_BUFS
    lib = _lib.load()
    nr, nc, th, tw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    cap = len(_TILE_PLAN_BUFS[0]) if _TILE_PLAN_BUFS else 64
    while True:
        if _TILE_PLAN_BUFS is None or len(_TILE_PLAN_BUFS[0]) < cap:
            _TILE_PLAN_BUFS = [(C.c_int32 * cap)() for _ in range(4)]
        ro, rb, co, cb = _TILE_PLAN_BUFS
        rc = lib.rt_det_tile_plan(int(h), int(w), int(tile), int(overlap), ro, rb, cap, co, cb, cap, C.byref(nr), C.byref(nc),
                                  C.byref(th), C.byref(tw))
        if rc == 8 and max(nr.value, nc.value) > cap:
            cap = 2 * max(nr.value, nc.value)
            continue
        _check(rc, None)
        return {"tile_h": th.value, "tile_w": tw.value, "row_origins": ro[:nr.value], "row_bounds": rb[:nr.value],
                "col_origins": co[:nc.value], "col_bounds": cb[:nc.value]}


_WINDOW_PLAN_BUFS = None   # the three output arrays of rec_window_plan, grown on demand, as det_tile_plan's


def rec_window_plan(L: int, window: int, overlap: int = 0) -> dict:
    """rt_rec_window_plan: the window plan (retto_amd/csrc/rec_windows.h) of a rec line of L columns, GPU-free: a dict with T,
    the line's time steps, and per unit its origin, width and ownership bound as lists (unit i covers the columns [origins[i],
    origins[i] + widths[i]) and owns the steps [bounds[i - 1], bounds[i]), from 0).  A line that is not windowed is one unit."""
    global _WINDOW_PLAN_BUFS
    lib = _lib.load()
    n, T = C.c_int(), C.c_int()
    cap = len(_WINDOW_PLAN_BUFS[0]) if _WINDOW_PLAN_BUFS else 64
    while True:
        if _WINDOW_PLAN_BUFS is None or len(_WINDOW_PLAN_BUFS[0]) < cap:
            _WINDOW_PLAN_BUFS = [(C.c_int32 * cap)() for _ in range(3)]
        o, w, b = _WINDOW_PLAN_BUFS
        rc = lib.rt_rec_window_plan(int(L), int(window), int(overlap), o, w, b, cap, C.byref(n), C.byref(T))
        if rc == 8 and n.value > cap:
            cap = 2 * n.value
            continue
        _check(rc, None)
        return {"T": T.value, "origins": o[:n.value], "widths": w[:n.value], "bounds": b[:n.value]}


def parse_dictionary(data: bytes) -> List[str]:
    """rt_parse_dictionary: RecCharacter::new (rec_processor.rs:29-46) -- "blank", the file's trimmed lines, " "."""
    lib = _lib.load()
    data = bytes(data)
    out, ln, n = C.c_void_p(), C.c_size_t(), C.c_int()
    err = C.create_string_buffer(256)
    rc = lib.rt_parse_dictionary(data, len(data), C.byref(out), C.byref(ln), C.byref(n), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)(err.value.decode("utf-8", "replace"))
    try:
        return C.string_at(out, ln.value).decode("utf-8").split("\n")
    finally:
        lib.rt_buffer_free(out)


class RettoSession:
    """RettoSession<RettoHipWorker> (session.rs:58-144), batched."""

    def __init__(self, cfg: RettoSessionConfig):
        self.config = cfg
        self._hd = _Handle(cfg)
        self.worker = RettoHipWorker(cfg, self._hd)
        self.worker.init()

    # -- stage functions ------------------------------------------------------------------
    def resize_both(self, img: np.ndarray) -> np.ndarray:
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape[:2]
        oh, ow = C.c_int(), C.c_int()
        _check(self._hd.lib.rt_resize_both_dims(self._hd.h, h, w, C.byref(oh), C.byref(ow)), self._hd.h)
        out = np.empty((oh.value, ow.value, 3), np.uint8)
        _check(self._hd.lib.rt_resize_both(self._hd.h, img.ctypes.data, h, w, out.ctypes.data, oh.value, ow.value), self._hd.h)
        return out

    def det_preprocess(self, img: np.ndarray) -> np.ndarray:
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape[:2]
        oh, ow = C.c_int(), C.c_int()
        _check(self._hd.lib.rt_det_input_dims(self._hd.h, h, w, C.byref(oh), C.byref(ow)), self._hd.h)
        out = np.empty((1, 3, oh.value, ow.value), np.float32)
        _check(self._hd.lib.rt_det_preprocess(self._hd.h, img.ctypes.data, h, w, out.ctypes.data), self._hd.h)
        return out

    def det_postprocess(self, pred: np.ndarray, ori_h: int, ori_w: int, max_out: int = 65536):
        pred = np.ascontiguousarray(pred, np.float32); h, w = pred.shape
        boxes = np.zeros((max_out, 8), np.float32); scores = np.zeros(max_out, np.float32); n = C.c_int()
        _check(self._hd.lib.rt_det_postprocess(self._hd.h, pred.ctypes.data, h, w, ori_h, ori_w, boxes.ctypes.data,
                                               scores.ctypes.data, max_out, C.byref(n)), self._hd.h)
        return boxes[:n.value].reshape(-1, 4, 2).copy(), scores[:n.value].copy()

    def crop_images(self, img: np.ndarray, boxes: np.ndarray, form: Optional[int] = None) -> List[np.ndarray]:
        """rt_crop_images; with form = 0 / 1 rt_debug_warp_crops: the same crops through the launch chosen -- 0 = one grid row
        per crop (k_warp_crops, what rt_crop_images runs), 1 = the flat pixel list (k_warp_crops_flat)."""
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape[:2]
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 8); n = len(b)
        ws = np.zeros(max(n, 1), np.int32); hs = np.zeros(max(n, 1), np.int32)
        _check(self._hd.lib.rt_crop_dims(b.ctypes.data, n, ws.ctypes.data, hs.ctypes.data), self._hd.h)
        total = int(sum(int(ws[i]) * int(hs[i]) * 3 for i in range(n)))
        out = np.zeros(max(total, 1), np.uint8)
        if form is None:
            rc = self._hd.lib.rt_crop_images(self._hd.h, img.ctypes.data, h, w, b.ctypes.data, n, out.ctypes.data, total)
        else:
            rc = self._hd.lib.rt_debug_warp_crops(self._hd.h, img.ctypes.data, h, w, b.ctypes.data, n, int(form), out.ctypes.data, total)
        _check(rc, self._hd.h)
        res, o = [], 0
        for i in range(n):
            sz = int(ws[i]) * int(hs[i]) * 3
            res.append(out[o:o + sz].reshape(int(hs[i]), int(ws[i]), 3).copy()); o += sz
        return res

    def resize_norm_image(self, crop: np.ndarray, ori_h: int, ori_w: int, img_h=48, img_w=320, max_wh_ratio=0.0):
        crop = np.ascontiguousarray(crop, np.uint8); h, w = crop.shape[:2]
        W = self._hd.lib.rt_resize_norm_width(img_h, img_w, max_wh_ratio)
        out = np.empty((3, img_h, W), np.float32)
        _check(self._hd.lib.rt_resize_norm_image(self._hd.h, crop.ctypes.data, h, w, ori_h, ori_w, img_h, img_w,
                                                 max_wh_ratio, out.ctypes.data), self._hd.h)
        return out

    def ctc_decode(self, probs: np.ndarray):
        probs = np.ascontiguousarray(probs, np.float32); n, t, c = probs.shape
        idx = np.zeros((n, t), np.int32); pr = np.zeros((n, t), np.float32)
        tok = np.zeros((n, t), np.int32); tn = np.zeros(n, np.int32); sc = np.zeros(n, np.float32)
        _check(self._hd.lib.rt_ctc_decode(self._hd.h, probs.ctypes.data, n, t, c, idx.ctypes.data, pr.ctypes.data,
                                          tok.ctypes.data, tn.ctypes.data, sc.ctypes.data), self._hd.h)
        return idx, pr, [tok[i, :tn[i]].copy() for i in range(n)], sc

    # -- pipeline ---------------------------------------------------------------------------
    @staticmethod
    def _page_arrays(pages, hs, ws, keep: list):
        """the rgb / hs / ws argument arrays of the batch entry points; host arrays that must outlive the call go to keep"""
        n = len(pages)
        arr_p = (C.c_void_p * max(n, 1))(); arr_h = (C.c_int * max(n, 1))(); arr_w = (C.c_int * max(n, 1))()
        for i, p in enumerate(pages):
            if isinstance(p, np.ndarray):
                p = np.ascontiguousarray(p, np.uint8); keep.append(p); arr_p[i] = p.ctypes.data
            else:
                arr_p[i] = int(p)
            arr_h[i], arr_w[i] = int(hs[i]), int(ws[i])
        return arr_p, arr_h, arr_w

    def run_batch_raw(self, pages, hs, ws, mem=RT_MEM_HOST, det_map_override=None, submit=False):
        """pages: sequence of host arrays or device pointers (ints). Returns an opaque results handle."""
        lib, h = self._hd.lib, self._hd.h
        n = len(pages)
        keep = []
        arr_p, arr_h, arr_w = self._page_arrays(pages, hs, ws, keep)
        ov = None
        if det_map_override is not None:
            ov = (C.c_void_p * max(n, 1))()
            for i, m in enumerate(det_map_override):
                if m is None:
                    ov[i] = None
                elif isinstance(m, np.ndarray):
                    m = np.ascontiguousarray(m, np.float32); keep.append(m); ov[i] = m.ctypes.data
                else:
                    ov[i] = int(m)
        out = C.c_void_p()
        if submit:   # rt_submit_batch: returns (ticket, the arrays that must stay alive until wait_batch)
            _check(lib.rt_submit_batch(h, arr_p, arr_h, arr_w, n, mem, ov, C.byref(out)), h)
            return out, keep
        _check(lib.rt_run_batch(h, arr_p, arr_h, arr_w, n, mem, ov, C.byref(out)), h)
        return out

    def submit_batch_raw(self, pages, hs, ws, mem=RT_MEM_HOST, det_map_override=None):
        """rt_submit_batch (the counterpart of RettoSession::run_stream's worker thread, session.rs:108-143): the batch is
        split over the session's lanes and this returns at once with a ticket; wait_batch_raw(ticket) gives the results
        handle.  Up to RT_MAX_INFLIGHT (8) batches ahead; nothing else may be called on the session in between."""
        return self.run_batch_raw(pages, hs, ws, mem, det_map_override, submit=True)

    def wait_batch_raw(self, ticket):
        t, _keep = ticket
        out = C.c_void_p()
        _check(self._hd.lib.rt_wait_batch(self._hd.h, t, C.byref(out)), self._hd.h)
        return out

    def _collect(self, r, page: int) -> RettoWorkerResult:
        lib = self._hd.lib
        n = lib.rt_results_count(r, page)
        boxes = np.ctypeslib.as_array(lib.rt_results_boxes(r, page), (n, 8)).copy() if n else np.zeros((0, 8), np.float32)
        ds = np.ctypeslib.as_array(lib.rt_results_det_scores(r, page), (n,)).copy() if n else np.zeros(0, np.float32)
        cl = np.ctypeslib.as_array(lib.rt_results_cls_labels(r, page), (n,)).copy() if n else np.zeros(0, np.uint16)
        cs = np.ctypeslib.as_array(lib.rt_results_cls_scores(r, page), (n,)).copy() if n else np.zeros(0, np.float32)
        rs = np.ctypeslib.as_array(lib.rt_results_rec_scores(r, page), (n,)).copy() if n else np.zeros(0, np.float32)
        det, cls, rec = [], [], []
        beam_on = self.rec_beam()[0] > 0   # (the setter is refused while a ticket is in flight: what the call ran under)
        for k in range(n):
            det.append(DetProcessorInnerResult(PointBox([Point(float(boxes[k, 2 * q]), float(boxes[k, 2 * q + 1]))
                                                         for q in range(4)]), float(ds[k])))
            cls.append(ClsProcessorSingleResult(ClsPostProcessLabel(int(cl[k]), float(cs[k]))))
            tp = C.POINTER(C.c_int32)()
            nt = lib.rt_results_rec_tokens(r, page, k, C.byref(tp))
            toks = np.ctypeslib.as_array(tp, (nt,)).copy() if nt else np.zeros(0, np.int32)
            words = self._words(r, page, k) if self.config.rec_processor_config.return_word_box else None
            cands, cols = self._candidates(r, page, k, nt)
            matches = self._lexicon_matches(r, page, k)
            snapped = None if matches is None else bool(lib.rt_results_rec_lexicon_snapped(r, page, k))
            rec.append(RecProcessorSingleResult(lib.rt_results_rec_text(r, page, k).decode("utf-8"), float(rs[k]), toks, words,
                                                cands, cols, matches, snapped, self._pattern(r, page, k),
                                                self._keywords(r, page, k), self._beams(r, page, k, beam_on),
                                                int(lib.rt_results_rec_windows(r, page, k)), self._flip(r, page, k)))
        return RettoWorkerResult(det, cls, rec)

    def _flip(self, r, page: int, k: int) -> Optional[RecFlip]:
        s0, s1 = C.c_float(), C.c_float()
        o = self._hd.lib.rt_results_rec_flip(r, page, k, C.byref(s0), C.byref(s1))
        return RecFlip(int(o), s0.value, s1.value) if o else None

    def _dictionary(self) -> List[str]:
        if getattr(self, "_dict", None) is None:
            src = self.config.rec_processor_config.character_source
            data = src.blob if src.path is None else open(src.path, "rb").read()
            self._dict = parse_dictionary(data)
        return self._dict

    def _candidates(self, r, page: int, line: int, n_tokens: int):
        if not self.config.rec_processor_config.return_candidates:
            return None, None
        cp = C.POINTER(_lib.Candidate)(); colp = C.POINTER(C.c_int32)()
        K = self._hd.lib.rt_results_rec_candidates(r, page, line, C.byref(cp), C.byref(colp))
        return _candidate_lists(cp, K, n_tokens, self._dictionary()), \
            (np.ctypeslib.as_array(colp, (n_tokens,)).copy() if n_tokens else np.zeros(0, np.int32))

    def _pattern(self, r, page: int, line: int):
        out = _lib.PatternResult()
        if not self._hd.lib.rt_results_rec_pattern(r, page, line, C.byref(out)):
            return None
        return bool(out.matched), float(out.logprob), float(out.free_logprob)

    def _keywords(self, r, page: int, line: int):
        lib = self._hd.lib
        kw = lib.rt_results_rec_keywords_id(r, page, line)
        if kw <= 0:
            return None
        hp = C.POINTER(_lib.KeywordHit)()
        n = lib.rt_results_rec_keywords(r, page, line, C.byref(hp))
        return [KeywordHit(int(hp[j].entry), lib.rt_keywords_entry_text(self._hd.h, kw, hp[j].entry).decode("utf-8"),
                           float(hp[j].score), int(hp[j].first_col), int(hp[j].last_col),
                           np.array(list(hp[j].quad), np.float32).reshape(4, 2)) for j in range(n)]

    def _beams(self, r, page: int, line: int, on: bool):
        if not on:
            return None
        lib = self._hd.lib
        bp = C.POINTER(_lib.Beam)()
        n = lib.rt_results_rec_beams(r, page, line, C.byref(bp))
        lp = C.POINTER(_lib.BeamLm)()
        fused = lib.rt_results_rec_beam_lm(r, page, line, C.byref(lp)) == n and bool(lp)
        vp = C.POINTER(_lib.BeamVocab)()
        worded = lib.rt_results_rec_beam_vocab(r, page, line, C.byref(vp)) == n and bool(vp)
        out = []
        for k in range(n):
            tp = C.POINTER(C.c_int32)()
            nt = lib.rt_results_rec_beam_tokens(r, page, line, k, C.byref(tp))
            out.append(BeamHypothesis(np.array([tp[i] for i in range(nt)], np.int32),
                                      lib.rt_results_rec_beam_text(r, page, line, k).decode("utf-8"), float(bp[k].logprob),
                                      float(lp[k].lm) if fused else None, float(lp[k].score) if fused else None,
                                      int(vp[k].oov_words) if worded else None, float(vp[k].score) if worded else None))
        return out

    def _lexicon_matches(self, r, page: int, line: int):
        lib = self._hd.lib
        lex = lib.rt_results_rec_lexicon_id(r, page, line)
        if lex <= 0:
            return None
        mp = C.POINTER(_lib.LexiconMatch)()
        n = lib.rt_results_rec_lexicon(r, page, line, C.byref(mp))
        return [(int(mp[j].entry), lib.rt_lexicon_entry_text(self._hd.h, lex, mp[j].entry).decode("utf-8"), float(mp[j].loglik),
                 float(mp[j].posterior)) for j in range(n)]

    def _words(self, r, page: int, line: int) -> List[RecWord]:
        lib = self._hd.lib
        wp = C.POINTER(_lib.Word)()
        nw = lib.rt_results_rec_words(r, page, line, C.byref(wp))
        return [_rec_word(wp[j], lib.rt_results_rec_word_text(r, page, line, j).decode("utf-8")) for j in range(nw)]

    def run_batch(self, pages: Sequence[np.ndarray], det_map_override=None) -> List[RettoWorkerResult]:
        pages = [np.ascontiguousarray(p, np.uint8) for p in pages]
        r = self.run_batch_raw(pages, [p.shape[0] for p in pages], [p.shape[1] for p in pages], RT_MEM_HOST,
                               det_map_override)
        try:
            self.last_det_checksum = self._hd.lib.rt_results_det_checksum(r)
            return [self._collect(r, i) for i in range(len(pages))]
        finally:
            self._hd.lib.rt_results_free(r)

    # -- det tiles --------------------------------------------------------------------------
    def set_det_tiles(self, tile: int, overlap: int = 64) -> None:
        """rt_set_det_tiles: pages whose det input is larger than ``tile`` either way are detected as overlapping tiles whose
        trusted parts are stitched into the one page map (retto_amd/csrc/det_tiles.h); 0 = off, the default.  tile: a multiple
        of 32, at least 64; overlap: a multiple of 32, at most tile / 2.  Holds for the pipeline calls that follow."""
        _check(self._hd.lib.rt_set_det_tiles(self._hd.h, int(tile), int(overlap)), self._hd.h)

    # -- rec beams --------------------------------------------------------------------------
    def set_rec_beam(self, beam: int, nbest: int = 1) -> None:
        """rt_set_rec_beam: every line of the pipeline calls that follow also reports its ``nbest`` most probable strings from a
        CTC prefix beam search of width ``beam`` (RecProcessorSingleResult.beams; retto_amd/csrc/ctc_beam.h).  beam = 0: off, the
        default; otherwise 1 <= beam <= MAX_BEAM and 1 <= nbest <= min(beam, MAX_NBEST).  It only reads a line: every other
        result stays what it is."""
        _check(self._hd.lib.rt_set_rec_beam(self._hd.h, int(beam), int(nbest)), self._hd.h)

    def rec_beam(self) -> Tuple[int, int]:
        """rt_rec_beam: (beam, nbest) as set; beam 0 = off."""
        b, n = C.c_int(), C.c_int()
        _check(self._hd.lib.rt_rec_beam(self._hd.h, C.byref(b), C.byref(n)), self._hd.h)
        return b.value, n.value

    # -- rec language model ------------------------------------------------------------------
    def create_lm(self, data, oov_log10: float = -7.0) -> int:
        """rt_lm_create: a character n-gram language model in ARPA text (str or bytes) over the session's dictionary
        (retto_amd/csrc/ctc_lm.h): a token is one dictionary entry, "<sp>" the space, "<s>" the line start.  oov_log10: the
        log10 probability of a class the model has no unigram for, unless the file has an "<unk>" unigram.  Returns the model's
        handle (0-based, valid for the session's life; at most MAX_LMS); see set_rec_beam_lm."""
        raw = data.encode("utf-8") if isinstance(data, str) else bytes(data)
        out = C.c_int()
        _check(self._hd.lib.rt_lm_create(self._hd.h, raw, len(raw), float(oov_log10), C.byref(out)), self._hd.h)
        return out.value

    def lm_info(self, lm: int) -> Optional[dict]:
        """rt_lm_info: {order, ngrams, dropped, states} of a language model; None for an unknown handle."""
        o, n, d, s = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if self._hd.lib.rt_lm_info(self._hd.h, int(lm), C.byref(o), C.byref(n), C.byref(d), C.byref(s)) != 0:
            return None
        return {"order": o.value, "ngrams": n.value, "dropped": d.value, "states": s.value}

    def set_rec_beam_lm(self, lm: int, alpha: float = 1.0, beta: float = 0.0) -> None:
        """rt_set_rec_beam_lm: the beam search of the pipeline calls that follow keeps, at every step, the candidates with the
        best logprob + (alpha * lm + beta * length) under model ``lm`` (BeamHypothesis.lm_logprob / lm_score); lm = -1: off, the
        default.  Without effect until set_rec_beam sets a beam.  alpha >= 0; both finite."""
        _check(self._hd.lib.rt_set_rec_beam_lm(self._hd.h, int(lm), float(alpha), float(beta)), self._hd.h)

    def rec_beam_lm(self) -> Tuple[int, float, float]:
        """rt_rec_beam_lm: (lm, alpha, beta) as set; lm -1 = off."""
        m, a, b = C.c_int(), C.c_float(), C.c_float()
        _check(self._hd.lib.rt_rec_beam_lm(self._hd.h, C.byref(m), C.byref(a), C.byref(b)), self._hd.h)
        return m.value, a.value, b.value

    # -- rec vocabulary ----------------------------------------------------------------------
    def create_vocab(self, words=(), ids=(), case_variants: bool = False) -> int:
        """rt_vocab_create: a word list for the beam search (retto_amd/csrc/ctc_vocab.h).  words: an iterable of str (each mapped
        code point by code point to the dictionary, as a lexicon's entries are) or one str / bytes of newline-separated words;
        ids: an iterable of class-id sequences that follow them.  case_variants: every text word also Capitalised and in UPPER
        CASE.  Returns the vocabulary's handle (0-based, valid for the session's life; at most MAX_VOCABS); see
        set_rec_beam_vocab."""
        if isinstance(words, (bytes, bytearray)):
            raw = bytes(words)
        else:
            raw = (words if isinstance(words, str) else "\n".join(words)).encode("utf-8")
        seqs = [np.asarray(w, np.int32).ravel() for w in ids]
        flat = np.ascontiguousarray(np.concatenate(seqs) if seqs else np.zeros(0, np.int32), np.int32)
        lens = np.ascontiguousarray([len(w) for w in seqs], np.int32)
        out = C.c_int()
        _check(self._hd.lib.rt_vocab_create(self._hd.h, raw, len(raw), flat.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
                                            len(seqs), _lib.VOCAB_CASE_VARIANTS if case_variants else 0, C.byref(out)), self._hd.h)
        return out.value

    def vocab_info(self, vocab: int) -> Optional[dict]:
        """rt_vocab_info: {words, nodes, word_classes, variants_dropped} of a vocabulary; None for an unknown handle."""
        w, n, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if self._hd.lib.rt_vocab_info(self._hd.h, int(vocab), C.byref(w), C.byref(n), C.byref(c), C.byref(d)) != 0:
            return None
        return {"words": w.value, "nodes": n.value, "word_classes": c.value, "variants_dropped": d.value}

    def set_rec_beam_vocab(self, vocab: int, gamma: float = 4.0) -> None:
        """rt_set_rec_beam_vocab: the beam search of the pipeline calls that follow charges every word of a hypothesis that is
        not in vocabulary ``vocab`` with ``gamma`` (BeamHypothesis.oov_words / vocab_score); characters the list does not spell
        with pass freely and separate words.  vocab = -1: off, the default.  Without effect until set_rec_beam sets a beam.
        gamma >= 0, finite.  The effect on accuracy with the real weights is not measured."""
        _check(self._hd.lib.rt_set_rec_beam_vocab(self._hd.h, int(vocab), float(gamma)), self._hd.h)

    def rec_beam_vocab(self) -> Tuple[int, float]:
        """rt_rec_beam_vocab: (vocab, gamma) as set; vocab -1 = off."""
        v, g = C.c_int(), C.c_float()
        _check(self._hd.lib.rt_rec_beam_vocab(self._hd.h, C.byref(v), C.byref(g)), self._hd.h)
        return v.value, g.value

    @property
    def det_tiles(self) -> Tuple[int, int]:
        """rt_det_tiles: (tile, overlap) as set; tile 0 = off."""
        t, o = C.c_int(), C.c_int()
        _check(self._hd.lib.rt_det_tiles(self._hd.h, C.byref(t), C.byref(o)), self._hd.h)
        return t.value, o.value

    def debug_det_tiles(self, rgb_det: np.ndarray):
        """rt_debug_det_tiles: the det stage of a one-page call on an RGB8 image at det-input size (both dimensions multiples
        of 32) under the session's det tiles.  Returns (tile_maps [n_rows * n_cols, tile_h, tile_w] in plan order, page_map
        [h, w], plan) with plan = det_tile_plan(h, w, *self.det_tiles)."""
        img = np.ascontiguousarray(rgb_det, np.uint8); h, w = img.shape[:2]
        tile, overlap = self.det_tiles
        plan = det_tile_plan(h, w, tile, overlap)
        n = len(plan["row_origins"]) * len(plan["col_origins"])
        tiles = np.empty((n, plan["tile_h"], plan["tile_w"]), np.float32); page = np.empty((h, w), np.float32)
        _check(self._hd.lib.rt_debug_det_tiles(self._hd.h, img.ctypes.data, h, w, tiles.ctypes.data, page.ctypes.data), self._hd.h)
        return tiles, page, plan

    # -- rec windows ------------------------------------------------------------------------
    def set_rec_windows(self, window: int, overlap: int = 0) -> None:
        """rt_set_rec_windows: rec lines at least 8 columns wider than ``window`` are read as overlapping windows whose trusted
        time steps are stitched into the one line's rows (retto_amd/csrc/rec_windows.h); 0 = off, the default.  window: a
        multiple of 32, at least 128; overlap: a multiple of 32, at most window / 2.  Holds for the pipeline calls that follow.
        The effect on accuracy with trained weights has not been measured."""
        _check(self._hd.lib.rt_set_rec_windows(self._hd.h, int(window), int(overlap)), self._hd.h)

    @property
    def rec_windows(self) -> Tuple[int, int]:
        """rt_rec_windows: (window, overlap) as set; window 0 = off."""
        w, o = C.c_int(), C.c_int()
        _check(self._hd.lib.rt_rec_windows(self._hd.h, C.byref(w), C.byref(o)), self._hd.h)
        return w.value, o.value

    def debug_rec_windows(self, lines: Sequence[np.ndarray]):
        """rt_debug_rec_windows: the lines ([3, 48, W_i] float32 each) as ONE rec group through the pipeline's own cut, network
        and stitch under the session's rec windows.  Returns (units, stitched, plans): units[i] = the list of line i's units as
        (idx [Tu], prob [Tu], z5 [Tu, 120]) in plan order, stitched[i] = (idx [T], prob [T], z5 [T, 120]) of line i, plans[i] =
        rec_window_plan(W_i, *self.rec_windows)."""
        lib = _lib.load()
        arrs = [np.ascontiguousarray(a, np.float32) for a in lines]
        for a in arrs:
            if a.ndim != 3 or a.shape[0] != 3 or a.shape[1] != 48:
                raise ValueError("debug_rec_windows: every line is [3, 48, W]")
        window, overlap = self.rec_windows
        widths = np.array([a.shape[2] for a in arrs], np.int32)
        plans = [rec_window_plan(int(w), window, overlap) for w in widths]
        unit_T = [[rec_window_plan(int(w), 0, 0)["T"] for w in p["widths"]] for p in plans]   # (a unit's own time steps)
        nu = sum(sum(t) for t in unit_T); nl = sum(p["T"] for p in plans)
        flat = np.concatenate([a.ravel() for a in arrs])
        u_idx = np.empty(max(nu, 1), np.int32); u_prob = np.empty(max(nu, 1), np.float32); u_z5 = np.empty((max(nu, 1), 120), np.float32)
        l_idx = np.empty(max(nl, 1), np.int32); l_prob = np.empty(max(nl, 1), np.float32); l_z5 = np.empty((max(nl, 1), 120), np.float32)
        _check(lib.rt_debug_rec_windows(self._hd.h, flat.ctypes.data, len(arrs), widths.ctypes.data, u_idx.ctypes.data, u_prob.ctypes.data,
                                        u_z5.ctypes.data, l_idx.ctypes.data, l_prob.ctypes.data, l_z5.ctypes.data), self._hd.h)
        units, stitched, uo, lo = [], [], 0, 0
        for p, ts in zip(plans, unit_T):
            us = []
            for t in ts:
                us.append((u_idx[uo:uo + t].copy(), u_prob[uo:uo + t].copy(), u_z5[uo:uo + t].copy())); uo += t
            units.append(us)
            stitched.append((l_idx[lo:lo + p["T"]].copy(), l_prob[lo:lo + p["T"]].copy(), l_z5[lo:lo + p["T"]].copy())); lo += p["T"]
        return units, stitched, plans

    # -- rec flip ---------------------------------------------------------------------------
    def set_rec_flip(self, cls_below: float) -> None:
        """rt_set_rec_flip: lines whose classifier score is below ``cls_below`` are read both ways up and the reading with the
        better greedy CTC score is kept (retto_amd/csrc/rec_flip.h); 0 = off, the default; above 1 = every line.  A both-ways
        line costs the rec network twice; with 0 < cls_below <= 1 every call syncs once more, for the classifier scores.  Holds
        for the pipeline calls that follow.  The effect on accuracy with trained weights has not been measured."""
        _check(self._hd.lib.rt_set_rec_flip(self._hd.h, float(cls_below)), self._hd.h)

    @property
    def rec_flip(self) -> float:
        """rt_rec_flip: cls_below as set; 0 = off."""
        v = C.c_float()
        _check(self._hd.lib.rt_rec_flip(self._hd.h, C.byref(v)), self._hd.h)
        return v.value

    def debug_rec_flip(self, crops: Sequence[np.ndarray], both: Sequence[int], max_wh_ratio: float) -> dict:
        """rt_debug_rec_flip: the crops ([h, w, 3] uint8 each) as ONE rec group through the pipeline's own rotate, resize_norm,
        network, score and select under the session's rec windows, every line at the padded width of ``max_wh_ratio``; both[i]:
        line i is read both ways.  Returns a dict: view_idx / view_prob [views, T] and view_z5 [views, T, 120] (the lines' view 0,
        then the flagged lines' view 1, in line order), view_ntok / view_score [views], view1 (line -> its view-1 index), taken [n], and the lines'
        final rows idx / prob [n, T] and z5 [n, T, 120]."""
        lib = _lib.load()
        arrs = [np.ascontiguousarray(a, np.uint8) for a in crops]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("debug_rec_flip: every crop is [h, w, 3]")
        n = len(arrs)
        flags = np.array([1 if b else 0 for b in both], np.uint8)
        if len(flags) != n:
            raise ValueError("debug_rec_flip: one flag per crop")
        hw = np.array([[a.shape[0], a.shape[1]] for a in arrs], np.int32).reshape(-1)
        flat = np.concatenate([a.ravel() for a in arrs]) if n else np.zeros(0, np.uint8)
        rh, rw = self.config.rec_processor_config.image_shape[1:3]
        W = int(lib.rt_resize_norm_width(int(rh), int(rw), float(max_wh_ratio)))
        T = rec_window_plan(W, 0, 0)["T"]
        nv = n + int(flags.sum())
        out = {"view_idx": np.empty((nv, T), np.int32), "view_prob": np.empty((nv, T), np.float32),
               "view_z5": np.empty((nv, T, 120), np.float32),
               "view_ntok": np.empty(nv, np.int32), "view_score": np.empty(nv, np.float32), "taken": np.empty(n, np.int32),
               "idx": np.empty((n, T), np.int32), "prob": np.empty((n, T), np.float32), "z5": np.empty((n, T, 120), np.float32)}
        _check(lib.rt_debug_rec_flip(self._hd.h, flat.ctypes.data, hw.ctypes.data, n, flags.ctypes.data, float(max_wh_ratio),
                                     *[out[k].ctypes.data for k in ("view_idx", "view_prob", "view_z5", "view_ntok", "view_score", "taken",
                                                                    "idx", "prob", "z5")]), self._hd.h)
        out["view1"] = {int(i): n + j for j, i in enumerate(np.flatnonzero(flags))}
        out["W"], out["T"] = W, T
        return out

    # -- rec charsets -----------------------------------------------------------------------
    def create_charset(self, text: str = "", ids: Sequence[int] = ()) -> int:
        """rt_charset_create: a set of classes a line's CTC decode may be restricted to -- the blank, every dictionary class
        whose whole entry is one character of ``text``, and the class ids ``ids``.  Returns its id (1-based, valid for the
        session's life; at most MAX_CHARSETS); see set_rec_charset and run_regions(charsets=...)."""
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        arr = (C.c_int32 * max(len(ids), 1))(*[int(i) for i in ids])
        out = C.c_int()
        _check(self._hd.lib.rt_charset_create(self._hd.h, raw, len(raw), arr, len(ids), C.byref(out)), self._hd.h)
        return out.value

    def charset_classes(self, charset: int) -> np.ndarray:
        """rt_charset_classes: the class ids of a charset in ascending order (empty for an unknown id)."""
        p = C.POINTER(C.c_int32)()
        n = self._hd.lib.rt_charset_classes(self._hd.h, int(charset), C.byref(p))
        return np.ctypeslib.as_array(p, (n,)).copy() if n else np.zeros(0, np.int32)

    def set_rec_charset(self, charset: int) -> None:
        """rt_set_rec_charset: the charset of every line of the pipeline calls that follow; 0 = none."""
        _check(self._hd.lib.rt_set_rec_charset(self._hd.h, int(charset)), self._hd.h)

    # -- rec lexicons -----------------------------------------------------------------------
    def create_lexicon(self, entries=(), ids=()) -> int:
        """rt_lexicon_create: a word list whose entries a line's result ranks by their CTC forward log-likelihood
        (RecProcessorSingleResult.lexicon_matches).  entries: strings, one entry each, read character by character (each the
        lowest class whose whole dictionary entry is that character); ids: entries given as lists of class ids, appended.
        Returns the lexicon's id (1-based, valid for the session's life; at most MAX_LEXICONS); see set_rec_lexicon and
        run_regions(lexicons=...)."""
        raw = bytes(_lexicon_text(entries))
        arr, lens, n_id = _lexicon_id_arrays(ids)
        out = C.c_int()
        _check(self._hd.lib.rt_lexicon_create(self._hd.h, raw, len(raw), arr, lens, n_id, C.byref(out)), self._hd.h)
        return out.value

    def lexicon_entries(self, lexicon: int) -> List[Tuple[List[int], str]]:
        """rt_lexicon_entries / _entry / _entry_text: every entry of a lexicon as (class ids, text); empty for an unknown id."""
        lib, h = self._hd.lib, self._hd.h
        out = []
        for e in range(lib.rt_lexicon_entries(h, int(lexicon))):
            p = C.POINTER(C.c_int32)()
            n = lib.rt_lexicon_entry(h, int(lexicon), e, C.byref(p))
            out.append(([int(p[i]) for i in range(n)], lib.rt_lexicon_entry_text(h, int(lexicon), e).decode("utf-8")))
        return out

    def set_rec_lexicon(self, lexicon: int) -> None:
        """rt_set_rec_lexicon: the lexicon of every line of the pipeline calls that follow; 0 = none."""
        _check(self._hd.lib.rt_set_rec_lexicon(self._hd.h, int(lexicon)), self._hd.h)

    def set_lexicon_snap(self, lexicon: int, min_posterior: float) -> None:
        """rt_lexicon_set_snap: from the next call on, a line that carries this lexicon and whose best entry's posterior reaches
        min_posterior takes that entry, aligned to its time steps, as its decode (RecProcessorSingleResult.lexicon_snapped;
        retto_amd/csrc/ctc_lexicon_align.h).  min_posterior in [0, 1]; 0 (the initial state) never snaps."""
        _check(self._hd.lib.rt_lexicon_set_snap(self._hd.h, int(lexicon), float(min_posterior)), self._hd.h)

    def lexicon_snap(self, lexicon: int) -> float:
        """rt_lexicon_snap: the lexicon's current min_posterior (0.0 for an unknown id)."""
        return float(self._hd.lib.rt_lexicon_snap(self._hd.h, int(lexicon)))

    # -- rec patterns -----------------------------------------------------------------------
    def create_pattern(self, pattern) -> int:
        """rt_pattern_create: a regular expression over the dictionary (retto_amd/csrc/ctc_pattern.h) that constrains the decode
        of the lines that carry it: "[0-9]{4}-[0-9]{2}-[0-9]{2}".  pattern: a string, or bytes to pass raw UTF-8.  Returns the
        pattern's id (1-based, valid for the session's life; at most MAX_PATTERNS); see set_rec_pattern and
        run_regions(patterns=...)."""
        raw = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        out = C.c_int()
        _check(self._hd.lib.rt_pattern_create(self._hd.h, raw, len(raw), C.byref(out)), self._hd.h)
        return out.value

    def pattern_info(self, pattern: int) -> Optional[dict]:
        """rt_pattern_info / rt_pattern_text: {text, states, pairs, min_steps} of a pattern; None for an unknown id."""
        S, P, ms = C.c_int(), C.c_int(), C.c_int()
        if self._hd.lib.rt_pattern_info(self._hd.h, int(pattern), C.byref(S), C.byref(P), C.byref(ms)) != 0:
            return None
        return {"text": self._hd.lib.rt_pattern_text(self._hd.h, int(pattern)).decode("utf-8", "replace"), "states": S.value,
                "pairs": P.value, "min_steps": ms.value}

    def set_rec_pattern(self, pattern: int) -> None:
        """rt_set_rec_pattern: the pattern of every line of the pipeline calls that follow; 0 = none."""
        _check(self._hd.lib.rt_set_rec_pattern(self._hd.h, int(pattern)), self._hd.h)

    # -- rec keywords -----------------------------------------------------------------------
    def create_keywords(self, entries=(), ids=(), min_score=float("-inf")) -> int:
        """rt_keywords_create: a keyword list whose entries are spotted inside every line that carries it
        (RecProcessorSingleResult.keywords; retto_amd/csrc/ctc_keyword.h).  entries / ids: as create_lexicon's.  min_score <= 0: a
        hit must score at least this; -inf reports the best hits whatever they score, 0 only where the greedy path holds the
        entry.  Returns the list's id (1-based, valid for the session's life; at most MAX_KEYWORD_LISTS); see set_rec_keywords
        and run_regions(keywords=...)."""
        raw = bytes(_lexicon_text(entries))
        arr, lens, n_id = _lexicon_id_arrays(ids)
        out = C.c_int(0)
        _check(self._hd.lib.rt_keywords_create(self._hd.h, raw, len(raw), arr, lens, n_id, float(min_score), C.byref(out)), self._hd.h)
        return out.value

    def keywords_entries(self, keywords: int) -> List[Tuple[List[int], str]]:
        """rt_keywords_entries / _entry / _entry_text: every entry of a keyword list as (class ids, text); empty for an unknown id."""
        lib, h = self._hd.lib, self._hd.h
        out = []
        for e in range(lib.rt_keywords_entries(h, int(keywords))):
            p = C.POINTER(C.c_int32)()
            n = lib.rt_keywords_entry(h, int(keywords), e, C.byref(p))
            out.append(([int(p[i]) for i in range(n)], lib.rt_keywords_entry_text(h, int(keywords), e).decode("utf-8")))
        return out

    def keywords_min_score(self, keywords: int) -> float:
        """rt_keywords_min_score: the list's min_score (NaN for an unknown id)."""
        return float(self._hd.lib.rt_keywords_min_score(self._hd.h, int(keywords)))

    def set_rec_keywords(self, keywords: int) -> None:
        """rt_set_rec_keywords: the keyword list of every line of the pipeline calls that follow; 0 = none."""
        _check(self._hd.lib.rt_set_rec_keywords(self._hd.h, int(keywords)), self._hd.h)

    def run_regions_raw(self, pages, hs, ws, quads, mem=RT_MEM_HOST, charsets=None, lexicons=None, patterns=None, keywords=None):
        """rt_run_regions.  pages: host arrays or device pointers (ints); quads[i]: the regions of page i, anything that
        reshapes to [n_i, 8] floats (TL, TR, BR, BL in original-page coordinates).  charsets (rt_run_regions_charsets): per
        page None or one id per region (-1 = the session default, 0 = unrestricted); lexicons (rt_run_regions_lexicons): the same for
        lexicon ids.  Returns an opaque results handle."""
        lib, h = self._hd.lib, self._hd.h
        n = len(pages)
        if len(quads) != n:
            raise InvalidArgument("run_regions: one list of quads per page")
        keep = []
        arr_p, arr_h, arr_w = self._page_arrays(pages, hs, ws, keep)
        arr_q = (C.c_void_p * max(n, 1))(); arr_n = (C.c_int * max(n, 1))()
        for i in range(n):
            q = np.ascontiguousarray(quads[i], np.float32).reshape(-1, 8); keep.append(q)
            arr_q[i] = q.ctypes.data if len(q) else None
            arr_n[i] = len(q)
        out = C.c_void_p()

        def id_arrays(per_page, what):
            if len(per_page) != n:
                raise InvalidArgument("run_regions: one list of %s ids per page (or None)" % what)
            arr_c = (C.c_void_p * max(n, 1))()
            for i in range(n):
                if per_page[i] is None:
                    arr_c[i] = None
                    continue
                c = np.ascontiguousarray(per_page[i], np.int32).reshape(-1); keep.append(c)
                if len(c) != arr_n[i]:
                    raise InvalidArgument("run_regions: page %d has %d regions but %d %s ids" % (i, arr_n[i], len(c), what))
                arr_c[i] = c.ctypes.data if len(c) else None
            return arr_c

        if keywords is not None:   # (rt_run_regions_keywords: any of the four may be missing)
            arrs = [id_arrays(v, what) if v is not None else None
                    for v, what in ((charsets, "charset"), (lexicons, "lexicon"), (patterns, "pattern"), (keywords, "keywords"))]
            _check(lib.rt_run_regions_keywords(h, arr_p, arr_h, arr_w, n, mem, arr_q, arr_n, arrs[0], arrs[1], arrs[2], arrs[3],
                                               C.byref(out)), h)
            return out
        if patterns is not None:   # (rt_run_regions_patterns: any of the three may be missing)
            arr_c = id_arrays(charsets, "charset") if charsets is not None else None
            arr_l = id_arrays(lexicons, "lexicon") if lexicons is not None else None
            _check(lib.rt_run_regions_patterns(h, arr_p, arr_h, arr_w, n, mem, arr_q, arr_n, arr_c, arr_l, id_arrays(patterns, "pattern"),
                                               C.byref(out)), h)
            return out
        if lexicons is not None:
            arr_c = id_arrays(charsets, "charset") if charsets is not None else None
            _check(lib.rt_run_regions_lexicons(h, arr_p, arr_h, arr_w, n, mem, arr_q, arr_n, arr_c, id_arrays(lexicons, "lexicon"),
                                               C.byref(out)), h)
            return out
        if charsets is not None:
            _check(lib.rt_run_regions_charsets(h, arr_p, arr_h, arr_w, n, mem, arr_q, arr_n, id_arrays(charsets, "charset"),
                                               C.byref(out)), h)
            return out
        _check(lib.rt_run_regions(h, arr_p, arr_h, arr_w, n, mem, arr_q, arr_n, C.byref(out)), h)
        return out

    def run_regions(self, pages: Sequence[np.ndarray], quads, charsets=None, lexicons=None, patterns=None,
                    keywords=None) -> List[RettoWorkerResult]:
        """The pipeline over regions the caller already knows (rt_run_regions): quads[i] = the [n_i, 4, 2] (or [n_i, 8]) quads
        of page i in original-page coordinates, TL, TR, BR, BL.  No detector runs; line k of a page is cut from the page as it
        is by quad k clamped to the page.  det_result holds the clamped quads with score 1.0.  charsets: per page None or one
        charset id per region (create_charset; -1 = the session default, 0 = unrestricted); lexicons: the same with lexicon
        ids (create_lexicon; 0 = none); patterns: the same with pattern ids (create_pattern; 0 = none; a region may not carry
        both a pattern and a lexicon); keywords: the same with keyword list ids (create_keywords; 0 = none; goes with anything)."""
        pages = [np.ascontiguousarray(p, np.uint8) for p in pages]
        r = self.run_regions_raw(pages, [p.shape[0] for p in pages], [p.shape[1] for p in pages], quads, charsets=charsets,
                                 lexicons=lexicons, patterns=patterns, keywords=keywords)
        try:
            self.last_det_checksum = self._hd.lib.rt_results_det_checksum(r)
            return [self._collect(r, i) for i in range(len(pages))]
        finally:
            self._hd.lib.rt_results_free(r)

    def run(self, image: Union[bytes, np.ndarray]) -> RettoWorkerResult:
        """session.rs:108-131.  ``image`` is an encoded image (bytes) or an RGB8 array."""
        if isinstance(image, (bytes, bytearray, memoryview)):
            return self.run_encoded_batch([bytes(image)])[0]
        return self.run_batch([image])[0]

    def run_encoded_batch(self, files: Sequence[bytes]) -> List[RettoWorkerResult]:
        """RettoSession::run over a batch of encoded images (rt_run_encoded_batch: decode on host threads, then
        the batch pipeline)."""
        n = len(files)
        files = [bytes(f) for f in files]
        ptrs = (C.c_char_p * n)(*files); lens = (C.c_size_t * n)(*[len(f) for f in files])
        out = C.c_void_p()
        _check(self._hd.lib.rt_run_encoded_batch(self._hd.h, ptrs, lens, n, None, None, C.byref(out)), self._hd.h)
        try:
            return [self._collect(out, i) for i in range(n)]
        finally:
            self._hd.lib.rt_results_free(out)

    def submit_encoded_batch(self, files: Sequence[bytes]):
        """rt_submit_encoded_batch: host entropy decoding inside the call, pixel reconstruction on the GPU ahead of the lanes.
        Returns a ticket for wait_batch_raw / wait_batch; the ticket owns the decoded data, the file bytes are not kept."""
        n = len(files)
        files = [bytes(f) for f in files]
        ptrs = (C.c_char_p * max(n, 1))(*files); lens = (C.c_size_t * max(n, 1))(*[len(f) for f in files])
        out = C.c_void_p()
        _check(self._hd.lib.rt_submit_encoded_batch(self._hd.h, ptrs, lens, n, C.byref(out)), self._hd.h)
        return out, []

    def wait_batch(self, ticket) -> List[RettoWorkerResult]:
        """wait_batch_raw, collected: one RettoWorkerResult per page."""
        r = self.wait_batch_raw(ticket)
        try:
            self.last_det_checksum = self._hd.lib.rt_results_det_checksum(r)
            return [self._collect(r, i) for i in range(self._hd.lib.rt_results_pages(r))]
        finally:
            self._hd.lib.rt_results_free(r)

    def decode_batch(self, files: Sequence[bytes]):
        """rt_decode_batch into host memory: (list of RGB8 [H,W,3] pages, list of on_device flags)."""
        n = len(files)
        files = [bytes(f) for f in files]
        ptrs = (C.c_char_p * max(n, 1))(*files); lens = (C.c_size_t * max(n, 1))(*[len(f) for f in files])
        hs = (C.c_int * max(n, 1))(); ws = (C.c_int * max(n, 1))(); dev = (C.c_int * max(n, 1))()
        lib, h = self._hd.lib, self._hd.h
        _check(lib.rt_decode_batch(h, ptrs, lens, n, hs, ws, None, RT_MEM_HOST, None), h)
        pages = [np.empty((hs[i], ws[i], 3), np.uint8) for i in range(n)]
        outs = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in pages])
        _check(lib.rt_decode_batch(h, ptrs, lens, n, hs, ws, outs, RT_MEM_HOST, dev), h)
        return pages, [bool(dev[i]) for i in range(n)]

    def run_stream(self, image, sender: Callable[[str, list], None]) -> None:
        """session.rs:133-143: emits ("Det", ...), ("Cls", ...), ("Rec", ...) in that order.  Det arrives while
        the crops are still being classified / read (rt_run_batch_stream); the payloads are the parsed
        RettoWorkerStageResult JSON of the stage."""
        import json
        page = decode_image(image) if isinstance(image, (bytes, bytearray, memoryview)) else np.ascontiguousarray(image, np.uint8)
        self.run_batch_stream([page], lambda _page, stage, payload: sender(stage, payload))

    def run_batch_stream(self, pages: Sequence[np.ndarray], on_stage: Callable[[int, str, list], None], det_map_override=None) -> None:
        """on_stage(page index, "Det" | "Cls" | "Rec", parsed stage JSON), called from the library's lane threads."""
        import json
        pages = [np.ascontiguousarray(p, np.uint8) for p in pages]
        n = len(pages)
        ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in pages])
        hs = (C.c_int * n)(*[p.shape[0] for p in pages]); ws = (C.c_int * n)(*[p.shape[1] for p in pages])
        maps = None
        if det_map_override is not None:
            keep = [None if m is None else np.ascontiguousarray(m, np.float32) for m in det_map_override]
            maps = (C.c_void_p * n)(*[None if m is None else m.ctypes.data for m in keep])
        errors = []

        def cb(_user, page, stage, js):
            try:
                on_stage(page, ("Det", "Cls", "Rec")[stage], json.loads(js.decode("utf-8")))
            except BaseException as e:  # never unwind through the C frames
                errors.append(e)

        ccb = _lib.STAGE_CALLBACK(cb)
        out = C.c_void_p()
        _check(self._hd.lib.rt_run_batch_stream(self._hd.h, ptrs, hs, ws, n, RT_MEM_HOST, maps, ccb, None, C.byref(out)), self._hd.h)
        self._hd.lib.rt_results_free(out)
        if errors:
            raise errors[0]

    def stage_json(self, page: np.ndarray) -> List[str]:
        """RettoWorkerStageResult JSON strings (Det, Cls, Rec) in retto-wasm's serde shape."""
        page = np.ascontiguousarray(page, np.uint8)
        r = self.run_batch_raw([page], [page.shape[0]], [page.shape[1]])
        try:
            return [self._hd.lib.rt_results_json(r, 0, s).decode("utf-8") for s in range(3)]
        finally:
            self._hd.lib.rt_results_free(r)

    # -- profiling --------------------------------------------------------------------------
    def profile_enable(self, on: bool = True):
        _check(self._hd.lib.rt_profile_enable(self._hd.h, int(on)), self._hd.h)

    def profile_get(self):
        names = C.POINTER(C.c_char_p)(); ms = C.POINTER(C.c_float)(); calls = C.POINTER(C.c_int)(); n = C.c_int()
        _check(self._hd.lib.rt_profile_get(self._hd.h, C.byref(names), C.byref(ms), C.byref(calls), C.byref(n)), self._hd.h)
        return {names[i].decode(): (float(ms[i]), int(calls[i])) for i in range(n.value)}

    def close(self):
        self._hd.close()


MODEL_DET, MODEL_CLS, MODEL_REC, MODEL_SDET, MODEL_SREC = 0, 1, 2, 3, 4   # (DET / REC sources also take the server .onnx files)


def onnx_to_rtwb(which: int, onnx_bytes: bytes) -> bytes:
    """PP-OCRv4 .onnx file -> RTWB blob (rt_onnx_to_rtwb; replaces ort_worker.rs:120-135's model loading).
    RettoSession accepts the .onnx bytes / path directly as well."""
    lib = _lib.load()
    out = C.c_void_p(); n = C.c_size_t(); err = C.create_string_buffer(1024)
    rc = lib.rt_onnx_to_rtwb(which, onnx_bytes, len(onnx_bytes), C.byref(out), C.byref(n), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, RettoError)(err.value.decode("utf-8", "replace"))
    try:
        return C.string_at(out, n.value)
    finally:
        lib.rt_buffer_free(out)


def model_manifest(which: int) -> str:
    lib = _lib.load()
    n = lib.rt_model_manifest(which, None, 0)
    buf = C.create_string_buffer(n)
    lib.rt_model_manifest(which, buf, n)
    return buf.value.decode()


def synthetic_session_config(seed: int = 0, device: int = 0, server: bool = False, **kw) -> RettoSessionConfig:
    """Session config over seeded synthetic PP-OCRv4-shaped weights (see retto_amd.synth): the mobile graphs, or with
    ``server=True`` the PP-OCRv4 server det / rec graphs (fp16 only: pass ``dtype="f16"``)."""
    from . import synth
    det, cls, rec, dic = synth.synth_server_models(seed) if server else synth.synth_models(seed)
    cfg = RettoSessionConfig(**kw)
    cfg.worker_config = RettoHipWorkerConfig(device=device, models=RettoWorkerModelProvider(
        det=RettoWorkerModelSource.Blob(det), rec=RettoWorkerModelSource.Blob(rec), cls=RettoWorkerModelSource.Blob(cls)))
    cfg.rec_processor_config.character_source = RettoWorkerModelSource.Blob(dic)
    return cfg

"""ctypes binding of libretto_hip.so (include/retto_hip.h).

There is no fallback: if the shared library is missing or cannot be loaded this
module raises, and every compute entry point fails with RT_ERR_BACKEND when no
gfx950 device is visible.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libretto_hip.so")

RT_OK = 0
RT_MEM_HOST, RT_MEM_DEVICE, RT_MEM_HOST_MAPS_DEVICE = 0, 1, 2
RT_MAX_INFLIGHT = 8   # include/retto_hip.h
RT_DTYPE_F32, RT_DTYPE_F16 = 0, 1
STATUS_NAMES = {0: "OK", 1: "IOError", 2: "ImageError", 3: "ShapeError", 4: "BackendError", 5: "Utf8Error",
                7: "ModelNotFoundError", 8: "InvalidArgument", 9: "CapacityError"}


class ModelSource(C.Structure):
    _fields_ = [("path", C.c_char_p), ("data", C.c_void_p), ("len", C.c_size_t)]


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32),
        ("det", ModelSource), ("cls", ModelSource), ("rec", ModelSource), ("dict", ModelSource),
        ("max_side_len", C.c_int32), ("min_side_len", C.c_int32),
        ("det_limit_side_len", C.c_int32), ("det_limit_type", C.c_int32),
        ("det_mean", C.c_float * 3), ("det_std", C.c_float * 3), ("det_scale", C.c_float),
        ("det_thresh", C.c_float), ("det_box_thresh", C.c_float), ("det_unclip_ratio", C.c_float),
        ("det_min_mini_box_size", C.c_int32), ("det_dilation", C.c_int32),
        ("cls_image_shape", C.c_int32 * 3), ("cls_batch_num", C.c_int32), ("cls_thresh", C.c_float),
        ("rec_image_shape", C.c_int32 * 3), ("rec_batch_num", C.c_int32),
        ("max_boxes_per_page", C.c_int32), ("det_sub_batch", C.c_int32), ("lanes", C.c_int32), ("dtype", C.c_int32),
        ("det_score_mode", C.c_int32), ("rec_return_candidates", C.c_int32), ("crop_source", C.c_int32),
        ("rec_return_word_box", C.c_int32),
    ]


class Word(C.Structure):   # rt_word
    _fields_ = [("quad", C.c_float * 8), ("first_token", C.c_int32), ("n_tokens", C.c_int32), ("first_col", C.c_int32),
                ("last_col", C.c_int32), ("kind", C.c_int32)]


class Candidate(C.Structure):   # rt_candidate
    _fields_ = [("id", C.c_int32), ("prob", C.c_float)]


MAX_CANDIDATES = 8   # RT_MAX_CANDIDATES
MAX_CHARSETS = 64    # RT_MAX_CHARSETS


class LexiconMatch(C.Structure):   # rt_lexicon_match
    _fields_ = [("entry", C.c_int32), ("loglik", C.c_float), ("posterior", C.c_float)]


class PatternResult(C.Structure):   # rt_pattern_result
    _fields_ = [("pattern", C.c_int32), ("matched", C.c_int32), ("logprob", C.c_float), ("free_logprob", C.c_float)]


class KeywordHit(C.Structure):   # rt_keyword_hit
    _fields_ = [("entry", C.c_int32), ("score", C.c_float), ("first_col", C.c_int32), ("last_col", C.c_int32), ("quad", C.c_float * 8)]


class Beam(C.Structure):   # rt_beam
    _fields_ = [("logprob", C.c_float), ("n_tokens", C.c_int32)]


class BeamLm(C.Structure):   # rt_beam_lm
    _fields_ = [("lm", C.c_float), ("score", C.c_float)]


class BeamVocab(C.Structure):   # rt_beam_vocab
    _fields_ = [("oov_words", C.c_int32), ("score", C.c_float)]


MAX_BEAM = 32                # RT_MAX_BEAM
VOCAB_MAX_LEN = 63           # RT_VOCAB_MAX_LEN
VOCAB_MAX_WORDS = 1 << 20    # RT_VOCAB_MAX_WORDS
MAX_VOCABS = 4               # RT_MAX_VOCABS
VOCAB_CASE_VARIANTS = 1      # RT_VOCAB_CASE_VARIANTS
MAX_LM_ORDER = 5             # RT_MAX_LM_ORDER
MAX_LM_NGRAMS = 1 << 22      # RT_MAX_LM_NGRAMS
MAX_LMS = 4                  # RT_MAX_LMS
MAX_NBEST = 8                # RT_MAX_NBEST
MAX_KEYWORD_LISTS = 16       # RT_MAX_KEYWORD_LISTS
KEYWORD_HITS = 8             # RT_KEYWORD_HITS
MAX_LEXICONS = 16            # RT_MAX_LEXICONS
LEXICON_MAX_ENTRIES = 65536  # RT_LEXICON_MAX_ENTRIES
LEXICON_MAX_LEN = 31         # RT_LEXICON_MAX_LEN
LEXICON_MATCHES = 4          # RT_LEXICON_MATCHES
MAX_PATTERNS = 16            # RT_MAX_PATTERNS
PATTERN_MAX_STATES = 64      # RT_PATTERN_MAX_STATES
PATTERN_MAX_PAIRS = 4096     # RT_PATTERN_MAX_PAIRS
PATTERN_MAX_BYTES = 1024     # RT_PATTERN_MAX_BYTES

# every symbol include/retto_hip.h declares (tests check that each is exported)
EXPORTS = [
    "rt_config_default", "rt_create", "rt_destroy", "rt_last_error", "rt_version",
    "rt_det", "rt_cls", "rt_rec", "rt_rec_ragged", "rt_rec_classes", "rt_model_info",
    "rt_resize_both_dims", "rt_resize_both", "rt_det_input_dims", "rt_det_preprocess", "rt_det_postprocess",
    "rt_crop_dims", "rt_crop_images", "rt_scale_and_clip", "rt_resize_norm_width", "rt_resize_norm_image",
    "rt_ctc_decode",
    "rt_run_batch", "rt_run_batch_stream", "rt_submit_batch", "rt_wait_batch", "rt_host_cpu_budget", "rt_results_free", "rt_results_pages", "rt_results_count", "rt_results_boxes",
    "rt_results_det_scores", "rt_results_cls_labels", "rt_results_cls_scores", "rt_results_rec_scores",
    "rt_results_rec_tokens", "rt_results_rec_text", "rt_results_rec_words", "rt_results_rec_word_text", "rt_debug_word_boxes", "rt_results_rec_candidates",
    "rt_debug_ctc_candidates", "rt_debug_ctc_candidates_host", "rt_results_det_checksum", "rt_results_json",
    "rt_device_malloc", "rt_device_free", "rt_memcpy_h2d", "rt_memcpy_d2h", "rt_synchronize",
    "rt_set_lanes", "rt_profile_enable", "rt_profile_get",
    "rt_onnx_to_rtwb", "rt_buffer_free", "rt_model_manifest", "rt_decode_image", "rt_run_encoded_batch",
    "rt_submit_encoded_batch", "rt_decode_batch", "rt_debug_jpeg_reconstruct",
    "rt_debug_set_variants", "rt_bench_gemm", "rt_bench_gemm_err", "rt_bench_lc", "rt_debug_conv16", "rt_debug_gemm", "rt_debug_dwconv", "rt_debug_dw_plan", "rt_debug_attention", "rt_debug_lc_block", "rt_debug_lc_wide", "rt_debug_conv13", "rt_debug_layernorm", "rt_debug_glue16", "rt_debug_conv16x", "rt_debug_fpn", "rt_debug_cls_block", "rt_debug_stem", "rt_debug_glue32", "rt_parse_dictionary", "rt_format_f32", "rt_rccl_unique_id", "rt_broadcast_blobs",
    "rt_run_regions", "rt_debug_warp_crops",
    "rt_charset_create", "rt_charset_classes", "rt_set_rec_charset", "rt_run_regions_charsets", "rt_debug_charset_compile",
    "rt_debug_ctc_charset", "rt_debug_ctc_charset_host",
    "rt_lexicon_create", "rt_lexicon_entries", "rt_lexicon_entry", "rt_lexicon_entry_text", "rt_set_rec_lexicon",
    "rt_run_regions_lexicons", "rt_results_rec_lexicon", "rt_results_rec_lexicon_id", "rt_debug_lexicon_compile",
    "rt_debug_ctc_lexicon", "rt_debug_ctc_lexicon_host",
    "rt_lexicon_set_snap", "rt_lexicon_snap", "rt_results_rec_lexicon_snapped", "rt_debug_ctc_lexicon_align",
    "rt_debug_ctc_lexicon_align_host",
    "rt_pattern_create", "rt_pattern_info", "rt_pattern_text", "rt_set_rec_pattern", "rt_run_regions_patterns", "rt_results_rec_pattern",
    "rt_debug_pattern_compile", "rt_debug_ctc_pattern", "rt_debug_ctc_pattern_host",
    "rt_keywords_create", "rt_keywords_entries", "rt_keywords_entry", "rt_keywords_entry_text", "rt_keywords_min_score",
    "rt_set_rec_keywords", "rt_run_regions_keywords", "rt_results_rec_keywords", "rt_results_rec_keywords_id", "rt_debug_ctc_keywords",
    "rt_debug_ctc_keywords_host", "rt_debug_span_quad",
    "rt_set_rec_beam", "rt_rec_beam", "rt_results_rec_beams", "rt_results_rec_beam_tokens", "rt_results_rec_beam_text",
    "rt_debug_ctc_beam", "rt_debug_ctc_beam_host",
    "rt_lm_create", "rt_lm_info", "rt_set_rec_beam_lm", "rt_rec_beam_lm", "rt_results_rec_beam_lm", "rt_debug_lm_compile",
    "rt_debug_lm_score", "rt_debug_ctc_beam_lm", "rt_debug_ctc_beam_lm_host",
    "rt_vocab_create", "rt_vocab_info", "rt_set_rec_beam_vocab", "rt_rec_beam_vocab", "rt_results_rec_beam_vocab",
    "rt_debug_vocab_compile", "rt_debug_vocab_walk", "rt_debug_ctc_beam_vocab", "rt_debug_ctc_beam_vocab_host",
    "rt_set_det_tiles", "rt_det_tiles", "rt_det_tile_plan", "rt_debug_det_tiles", "rt_debug_arena_high_water", "rt_bench_memcpy_d2d",
    "rt_set_rec_windows", "rt_rec_windows", "rt_rec_window_plan", "rt_results_rec_windows", "rt_debug_rec_windows",
    "rt_set_rec_flip", "rt_rec_flip", "rt_rec_flip_choose", "rt_results_rec_flip", "rt_debug_rec_flip",
]

STAGE_CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_char_p)  # rt_stage_callback

_lib = None


def source_digest() -> str:
    """sha256 over the kernel / host sources of libretto_hip (retto_amd/csrc/*.hip, *.cpp, *.h and the public header): what a
    committed profile (profiles/pmc_traffic.json) was collected on.  Content-based, so it is the same in a git checkout and in
    the snapshot a GPU box receives (which has no .git)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.cpp")) +
                   glob.glob(os.path.join(_HERE, "csrc", "*.h")) + [os.path.join(os.path.dirname(_HERE), "include", "retto_hip.h")])
    for f in files:
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def load():
    """Loads the HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C retto_amd/csrc` (python -c 'import __graft_entry__ as g; "
            "g.build()'). retto_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_last_error.argtypes = [C.c_void_p]
    lib.rt_version.restype = C.c_char_p
    lib.rt_create.argtypes = [P(Config), P(C.c_void_p)]
    lib.rt_destroy.argtypes = [C.c_void_p]
    lib.rt_destroy.restype = None
    lib.rt_results_free.argtypes = [C.c_void_p]
    lib.rt_results_free.restype = None
    lib.rt_results_boxes.restype = P(C.c_float)
    lib.rt_results_det_scores.restype = P(C.c_float)
    lib.rt_results_cls_labels.restype = P(C.c_uint16)
    lib.rt_results_cls_scores.restype = P(C.c_float)
    lib.rt_results_rec_scores.restype = P(C.c_float)
    lib.rt_results_rec_text.restype = C.c_char_p
    lib.rt_results_json.restype = C.c_char_p
    lib.rt_results_det_checksum.restype = C.c_double
    for name in ("rt_results_boxes", "rt_results_det_scores", "rt_results_cls_labels", "rt_results_cls_scores",
                 "rt_results_rec_scores", "rt_results_count"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int]
    lib.rt_results_pages.argtypes = [C.c_void_p]
    lib.rt_results_det_checksum.argtypes = [C.c_void_p]
    lib.rt_results_rec_tokens.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(C.c_int32))]
    lib.rt_results_rec_text.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_results_json.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_scale_and_clip.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.rt_resize_norm_width.argtypes = [C.c_int, C.c_int, C.c_float]
    lib.rt_device_malloc.argtypes = [C.c_void_p, C.c_size_t, P(C.c_void_p)]
    lib.rt_device_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.rt_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.rt_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.rt_synchronize.argtypes = [C.c_void_p]
    lib.rt_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.rt_set_lanes.argtypes = [C.c_void_p, C.c_int]
    lib.rt_det.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.rt_cls.argtypes = lib.rt_det.argtypes
    lib.rt_rec.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, P(C.c_int)]
    lib.rt_rec_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(C.c_int), C.c_void_p, P(C.c_int)]
    lib.rt_rec_classes.argtypes = [C.c_void_p]
    lib.rt_resize_both_dims.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_int), P(C.c_int)]
    lib.rt_det_input_dims.argtypes = lib.rt_resize_both_dims.argtypes
    lib.rt_resize_both.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.rt_det_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.rt_det_postprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, P(C.c_int)]
    lib.rt_crop_dims.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.rt_crop_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_size_t]
    lib.rt_resize_norm_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_float, C.c_void_p]
    lib.rt_ctc_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_run_batch.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p),
                                 P(C.c_void_p)]
    lib.rt_submit_batch.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p), P(C.c_void_p)]
    lib.rt_wait_batch.argtypes = [C.c_void_p, C.c_void_p, P(C.c_void_p)]
    lib.rt_run_regions.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p), P(C.c_int),
                                   P(C.c_void_p)]
    lib.rt_debug_warp_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_size_t]
    lib.rt_run_batch_stream.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p),
                                        STAGE_CALLBACK, C.c_void_p, P(C.c_void_p)]
    lib.rt_profile_get.argtypes = [C.c_void_p, P(P(C.c_char_p)), P(P(C.c_float)), P(P(C.c_int)), P(C.c_int)]
    lib.rt_onnx_to_rtwb.argtypes = [C.c_int, C.c_void_p, C.c_size_t, P(C.c_void_p), P(C.c_size_t), C.c_char_p, C.c_size_t]
    lib.rt_buffer_free.argtypes = [C.c_void_p]
    lib.rt_buffer_free.restype = None
    lib.rt_model_manifest.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    lib.rt_decode_image.argtypes = [C.c_char_p, C.c_size_t, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_char_p, C.c_size_t]
    lib.rt_run_encoded_batch.argtypes = [C.c_void_p, P(C.c_char_p), P(C.c_size_t), C.c_int, C.c_void_p, C.c_void_p, P(C.c_void_p)]
    lib.rt_submit_encoded_batch.argtypes = [C.c_void_p, P(C.c_char_p), P(C.c_size_t), C.c_int, P(C.c_void_p)]
    lib.rt_decode_batch.argtypes = [C.c_void_p, P(C.c_char_p), P(C.c_size_t), C.c_int, P(C.c_int), P(C.c_int), P(C.c_void_p),
                                    C.c_int, P(C.c_int)]
    lib.rt_debug_jpeg_reconstruct.argtypes = [C.c_char_p, C.c_size_t, P(C.c_void_p), P(C.c_int), P(C.c_int), P(C.c_int),
                                              C.c_char_p, C.c_size_t]
    lib.rt_model_manifest.restype = C.c_size_t
    lib.rt_parse_dictionary.argtypes = [C.c_char_p, C.c_size_t, P(C.c_void_p), P(C.c_size_t), P(C.c_int), C.c_char_p, C.c_size_t]
    lib.rt_results_rec_words.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(Word))]
    lib.rt_results_rec_word_text.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.rt_results_rec_word_text.restype = C.c_char_p
    lib.rt_debug_word_boxes.argtypes = [C.c_char_p, C.c_size_t, P(C.c_int32), P(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int,
                                        P(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(Word), P(C.c_int)]
    lib.rt_debug_gemm.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_dwconv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.rt_debug_attention.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.rt_debug_lc_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                      C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    lib.rt_debug_dw_plan.argtypes = [C.c_int] * 8 + [C.c_void_p]
    lib.rt_debug_lc_wide.argtypes = ([C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                     C.c_float, C.c_float] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p, C.c_longlong] * 3 + [C.c_void_p])
    lib.rt_debug_conv13.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.rt_debug_layernorm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                       C.c_void_p]
    lib.rt_debug_glue16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p,
                                    C.c_longlong]
    lib.rt_debug_fpn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_conv16x.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong,
                                     C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                     C.c_longlong, C.c_void_p]
    lib.rt_debug_cls_block.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 10 + [C.c_void_p] * 10 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.rt_debug_stem.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    lib.rt_debug_glue32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong,
                                    C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.rt_results_rec_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(Candidate)), P(P(C.c_int32))]
    lib.rt_debug_ctc_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_candidates_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_charset_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, P(C.c_int32), C.c_int, P(C.c_int)]
    lib.rt_charset_classes.argtypes = [C.c_void_p, C.c_int, P(P(C.c_int32))]
    lib.rt_set_rec_charset.argtypes = [C.c_void_p, C.c_int]
    lib.rt_run_regions_charsets.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p),
                                            P(C.c_int), P(C.c_void_p), P(C.c_void_p)]
    lib.rt_debug_charset_compile.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, P(C.c_int32), C.c_int, C.c_void_p,
                                             C.c_int, P(C.c_int), C.c_char_p, C.c_size_t]
    lib.rt_debug_ctc_charset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_charset_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_lexicon_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, P(C.c_int32), P(C.c_int32), C.c_int, P(C.c_int)]
    lib.rt_lexicon_entries.argtypes = [C.c_void_p, C.c_int]
    lib.rt_lexicon_entry.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(C.c_int32))]
    lib.rt_lexicon_entry_text.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_lexicon_entry_text.restype = C.c_char_p
    lib.rt_set_rec_lexicon.argtypes = [C.c_void_p, C.c_int]
    lib.rt_run_regions_lexicons.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p),
                                            P(C.c_int), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p)]
    lib.rt_results_rec_lexicon.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(LexiconMatch))]
    lib.rt_results_rec_lexicon_id.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_debug_lexicon_compile.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, P(C.c_int32), P(C.c_int32), C.c_int,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int),
                                             C.c_char_p, C.c_size_t]
    lib.rt_debug_ctc_lexicon.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_lexicon_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_lexicon_set_snap.argtypes = [C.c_void_p, C.c_int, C.c_float]
    lib.rt_lexicon_snap.argtypes = [C.c_void_p, C.c_int]
    lib.rt_lexicon_snap.restype = C.c_float
    lib.rt_results_rec_lexicon_snapped.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_debug_ctc_lexicon_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_lexicon_align_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_pattern_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, P(C.c_int)]
    lib.rt_pattern_info.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int)]
    lib.rt_pattern_text.argtypes = [C.c_void_p, C.c_int]
    lib.rt_pattern_text.restype = C.c_char_p
    lib.rt_set_rec_pattern.argtypes = [C.c_void_p, C.c_int]
    lib.rt_run_regions_patterns.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p),
                                            P(C.c_int), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p)]
    lib.rt_results_rec_pattern.argtypes = [C.c_void_p, C.c_int, C.c_int, P(PatternResult)]
    lib.rt_debug_pattern_compile.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int),
                                             C.c_char_p, C.c_size_t]
    lib.rt_debug_ctc_pattern.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_pattern_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_keywords_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, P(C.c_int32), P(C.c_int32), C.c_int, C.c_float, P(C.c_int)]
    lib.rt_keywords_entries.argtypes = [C.c_void_p, C.c_int]
    lib.rt_keywords_entry.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(C.c_int32))]
    lib.rt_keywords_entry_text.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_keywords_entry_text.restype = C.c_char_p
    lib.rt_keywords_min_score.argtypes = [C.c_void_p, C.c_int]
    lib.rt_keywords_min_score.restype = C.c_float
    lib.rt_set_rec_keywords.argtypes = [C.c_void_p, C.c_int]
    lib.rt_run_regions_keywords.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), C.c_int, C.c_int, P(C.c_void_p),
                                            P(C.c_int), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p)]
    lib.rt_results_rec_keywords.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(KeywordHit))]
    lib.rt_results_rec_keywords_id.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_debug_ctc_keywords.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_keywords_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
    lib.rt_debug_span_quad.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p]
    lib.rt_set_rec_beam.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_rec_beam.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int)]
    lib.rt_results_rec_beams.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(Beam))]
    lib.rt_results_rec_beam_tokens.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, P(P(C.c_int32))]
    lib.rt_results_rec_beam_text.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.rt_results_rec_beam_text.restype = C.c_char_p
    lib.rt_debug_ctc_beam.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_beam_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_lm_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_float, P(C.c_int)]
    lib.rt_lm_info.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int)]
    lib.rt_set_rec_beam_lm.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
    lib.rt_rec_beam_lm.argtypes = [C.c_void_p, P(C.c_int), P(C.c_float), P(C.c_float)]
    lib.rt_results_rec_beam_lm.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(BeamLm))]
    lib.rt_debug_lm_compile.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int),
                                        P(C.c_float), P(C.c_int), C.c_char_p, C.c_size_t]
    lib.rt_debug_lm_score.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    lib.rt_debug_ctc_beam_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                         C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_beam_lm_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_vocab_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, P(C.c_int)]
    lib.rt_vocab_info.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int)]
    lib.rt_set_rec_beam_vocab.argtypes = [C.c_void_p, C.c_int, C.c_float]
    lib.rt_rec_beam_vocab.argtypes = [C.c_void_p, P(C.c_int), P(C.c_float)]
    lib.rt_results_rec_beam_vocab.argtypes = [C.c_void_p, C.c_int, C.c_int, P(P(BeamVocab))]
    lib.rt_debug_vocab_compile.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int),
                                           C.c_char_p, C.c_size_t]
    lib.rt_debug_vocab_walk.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_char_p, C.c_size_t]
    lib.rt_debug_ctc_beam_vocab.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                            C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    lib.rt_debug_ctc_beam_vocab_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float,
                                                 C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
    lib.rt_set_det_tiles.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_det_tiles.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int)]
    lib.rt_det_tile_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32), C.c_int, P(C.c_int32), P(C.c_int32),
                                     C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int)]
    lib.rt_debug_det_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.rt_debug_arena_high_water.argtypes = [C.c_void_p, P(C.c_longlong)]
    lib.rt_bench_memcpy_d2d.argtypes = [C.c_void_p, C.c_size_t, C.c_int, P(C.c_float)]
    lib.rt_set_rec_windows.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_rec_windows.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int)]
    lib.rt_rec_window_plan.argtypes = [C.c_int, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32), P(C.c_int32), C.c_int, P(C.c_int), P(C.c_int)]
    lib.rt_results_rec_windows.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.rt_debug_rec_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.rt_set_rec_flip.argtypes = [C.c_void_p, C.c_float]
    lib.rt_rec_flip.argtypes = [C.c_void_p, P(C.c_float)]
    lib.rt_rec_flip_choose.argtypes = [C.c_int, C.c_float, C.c_int, C.c_float]
    lib.rt_results_rec_flip.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_float), P(C.c_float)]
    lib.rt_debug_rec_flip.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float] + [C.c_void_p] * 9
    _lib = lib
    return lib

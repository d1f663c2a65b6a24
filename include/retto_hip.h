/*
 * retto_hip.h -- C ABI of libretto_hip.so, the MI355X (gfx950) backend for
 * retto-core's OCR hot path.  Plain pointers and sizes only; no C++/torch types.
 *
 * What each entry point replaces in the reference (paths relative to
 * /root/reference):
 *
 *   L1 tensor-level worker  (trait RettoInnerWorker, retto-core/src/worker.rs:69-73;
 *                            ORT implementation retto-core/src/worker/ort_worker.rs:189-220)
 *       rt_det / rt_cls / rt_rec
 *   worker construction     (trait RettoWorker::new/init, worker.rs:91-98; model source
 *                            resolution worker.rs:18-56; ort_worker.rs:120-181)
 *       rt_create / rt_destroy
 *   L2 pipeline             (RettoSession::run / run_stream, retto-core/src/session.rs:75-143)
 *       rt_run_batch (+ rt_results_* accessors); stage order Det -> Cls -> Rec
 *   stage functions, exported so each row of SURVEY.md section 8(a) can be checked
 *   against the oracle on its own:
 *       rt_resize_both        ImageHelper::resize_both            image_helper.rs:106-148   (a2)
 *       rt_det_preprocess     DetProcessor::preprocess            det_processor.rs:256-274  (a3)
 *       rt_det_postprocess    DetProcessor::postprocess           det_processor.rs:279-335  (a5)
 *       rt_crop_images        ImageHelper::get_crop_img           image_helper.rs:223-249   (a6)
 *       rt_scale_and_clip     PointBox::scale_and_clip            points.rs:179-194         (a7)
 *       rt_resize_norm_image  ImageHelper::resize_norm_image      image_helper.rs:176-209   (a8/a10)
 *       rt_ctc_decode         RecProcessor::postprocess + decode  rec_processor.rs:48-97,190-208 (a12)
 *
 * Error convention (retto-core/src/error.rs:2-21): every call returns an rt_status;
 * rt_last_error() gives the message of the last failure on that session (or of the
 * last failed rt_create on this thread when session == NULL).
 *
 * Threading (worker.rs:70-72, session.rs:108,133 take &mut self): one call in flight
 * per session; sessions are independent (one per GPU); a session may be used from a
 * thread other than the one that created it.
 *
 * Ownership: caller-owned inputs stay caller-owned; outputs are written into
 * caller-allocated buffers, except rt_results which is library-owned until
 * rt_results_free().
 *
 * All computation happens on the GPU.  There is no CPU fallback: if no gfx950 device
 * is visible rt_create fails with RT_ERR_BACKEND.
 */
#ifndef RETTO_HIP_H
#define RETTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_API __attribute__((visibility("default")))

typedef enum rt_status {
  RT_OK = 0,
  RT_ERR_IO = 1,              /* RettoError::IOError */
  RT_ERR_IMAGE = 2,           /* RettoError::ImageError */
  RT_ERR_SHAPE = 3,           /* RettoError::ShapeError */
  RT_ERR_BACKEND = 4,         /* RettoError::OrtError's slot: HIP / device failures */
  RT_ERR_UTF8 = 5,            /* RettoError::Utf8Error */
  RT_ERR_MODEL_NOT_FOUND = 7, /* RettoError::ModelNotFoundError */
  RT_ERR_INVALID = 8,         /* NULL / out-of-range argument */
  RT_ERR_CAPACITY = 9         /* a device-side work list overflowed its configured capacity */
} rt_status;

/* RettoWorkerModelSource::{Path,Blob} (worker.rs:18-27): path != NULL selects Path,
 * otherwise (data,len) is a Blob.  A missing path or an empty blob is
 * RT_ERR_MODEL_NOT_FOUND (worker.rs:33-47).  Model format: RTWB (retto_amd/synth.py). */
typedef struct rt_model_source {
  const char* path;
  const void* data;
  size_t len;
} rt_model_source;

/* RettoSessionConfig + Det/Cls/RecProcessorConfig defaults (session.rs:28-39,
 * det_processor.rs:75-93, cls_processor.rs:27-36, rec_processor.rs:111-136). */
typedef struct rt_config {
  uint32_t struct_size;      /* sizeof(rt_config) of the header the caller was compiled against: set by rt_config_default,
                                checked by rt_create (a host built against an older, shorter struct gets RT_ERR_INVALID instead
                                of having fields read past the end of its struct) */
  int32_t device_id;         /* HIP device ordinal (RettoOrtWorkerDevice::Cuda(id) analogue) */
  rt_model_source det, cls, rec, dict;
  int32_t max_side_len;      /* 2000 */
  int32_t min_side_len;      /* 30 */
  /* det */
  int32_t det_limit_side_len; /* 736 */
  int32_t det_limit_type;     /* 0 = Min (default), 1 = Max */
  float det_mean[3];          /* 0.5 */
  float det_std[3];           /* 0.5 */
  float det_scale;            /* 1/255 */
  float det_thresh;           /* 0.3 */
  float det_box_thresh;       /* 0.5 */
  float det_unclip_ratio;     /* 1.6 */
  int32_t det_min_mini_box_size; /* 3 */
  int32_t det_dilation;       /* 1 = 2x2 ones kernel (default), 0 = none */
  /* cls */
  int32_t cls_image_shape[3]; /* 3,48,192 */
  int32_t cls_batch_num;      /* 6 */
  float cls_thresh;           /* 0.9 */
  /* rec */
  int32_t rec_image_shape[3]; /* 3,48,320 */
  int32_t rec_batch_num;      /* 6 */
  /* backend knobs (no reference counterpart) */
  int32_t max_boxes_per_page; /* capacity of the per-page box list (the reference's list is unbounded); 0 = default 8192, at most 65536 */
  int32_t det_sub_batch;      /* pages per det launch group; 0 = default */
  int32_t lanes;              /* concurrent page streams inside rt_run_batch (1..4); 0 = default 3 */
  int32_t dtype;              /* rt_dtype: arithmetic of the three networks.  RT_DTYPE_F32 (default) = what the reference's
                                 ort-CPU path computes in; RT_DTYPE_F16 = fp16 storage / MFMA, fp32 accumulation
                                 (BASELINE.json config 5).  The PP-OCRv4 server graphs are built in fp16 only. */
  int32_t det_score_mode;     /* 0 = Fast (default), 1 = Slow: DetProcessorConfig::score_mode (det_processor.rs:22-31,69).  Slow
                                 scores a box by the mean over the contour's own polygon (its full point chain) instead of its
                                 min-area rect, as the field's doc comment specifies; the reference itself never reads the field
                                 and computes Fast either way.  rt_create rejects other values with RT_ERR_INVALID. */
  int32_t rec_return_candidates; /* 0 = off (default); K = 1 .. RT_MAX_CANDIDATES: per kept token its time step, its own
                                 probability and the K - 1 next best classes (rt_results_rec_candidates).  The reference has no
                                 counterpart (rec_processor.rs:155 `// TODO: word_results`).  Off: no extra launch, no extra
                                 workspace.  rt_create rejects other values with RT_ERR_INVALID. */
  int32_t crop_source;        /* where the text lines are cut from.  0 = Resized (default): from the page after resize_both, as the
                                 reference does (session.rs:75-106, image_helper.rs:223-249).  1 = Original: line k of a page is
                                 get_crop_img(the caller's page, rt_results_boxes(page)[k]) -- the page as handed in (or decoded) at
                                 ori_h x ori_w, and the quad the results report, i.e. after scale_and_clip.  The crop size, the
                                 rotate270 decision, the homography, the cls / rec ordering by aspect and the running max_wh_ratio
                                 are all computed from that quad by unchanged arithmetic; detection, DB post-processing, the
                                 reported boxes and their scores are untouched; word boxes map back through the same homography
                                 and are scale_and_clip'd with the original size on both sides.  A page resize_both leaves as it
                                 is gives bit-identical results in both modes.  The crops are warped by a launch over the flat
                                 list of output pixels (crop area grows with the square of the resize ratio, and differs by
                                 orders of magnitude between lines).  No reference counterpart (PaddleOCR crops from the image it
                                 was given).  Applies to every entry point that runs the pipeline.  rt_create rejects other values
                                 with RT_ERR_INVALID. */
  int32_t rec_return_word_box; /* 0 = off (default), 1 = word boxes (rt_results_rec_words): RecCharacter::decode's
                                 `return_word_box` (rec_processor.rs:48-56), which the reference declares but never implements
                                 (its only caller passes false, :199-206).  Off: no extra launch and no extra workspace.
                                 rt_create rejects other values with RT_ERR_INVALID. */
} rt_config;
#define RT_MAX_CANDIDATES 8
typedef enum rt_dtype { RT_DTYPE_F32 = 0, RT_DTYPE_F16 = 1 } rt_dtype;

typedef struct rt_session rt_session;
typedef struct rt_results rt_results;

RT_API void rt_config_default(rt_config* cfg);
RT_API int rt_create(const rt_config* cfg, rt_session** out);
RT_API void rt_destroy(rt_session* s);
RT_API const char* rt_last_error(const rt_session* s);
RT_API const char* rt_version(void);

/* ---- L1: RettoInnerWorker (host tensors in, host tensors out) ------------------- */
/* det: f32 NCHW [n,3,h,w] (h,w multiples of 32) -> f32 [n,1,h,w] */
RT_API int rt_det(rt_session* s, const float* nchw, int n, int c, int h, int w, float* out);
/* cls: f32 [n,3,48,192] -> f32 [n,2] (softmax) */
RT_API int rt_cls(rt_session* s, const float* nchw, int n, int c, int h, int w, float* out);
/* rec: f32 [n,3,48,w] -> f32 [n,T,6625] (softmax); *t_out = T; call with out == NULL to
 * query T only. */
RT_API int rt_rec(rt_session* s, const float* nchw, int n, int c, int h, int w, float* out, int* t_out);
/* rec over lines of DIFFERENT widths in one launch series: line i is f32 [3,48,widths[i]] (lines concatenated); out = the lines'
 * [T_i,6625] softmax rows concatenated, t_out[i] = T_i (out == NULL: query the T_i only).  No reference counterpart as a worker
 * call (ort_worker.rs:211-220 takes one width per call); it is the tensor-level view of what rt_run_batch does with
 * rec_processor.rs:214-270's batches -- each keeps the width the running max_wh_ratio gives it, all in one ragged launch group --
 * so that the parity tests can compare exactly that form with the oracle, line by line. */
RT_API int rt_rec_ragged(rt_session* s, const float* nchw, int n, const int* widths, float* out, int* t_out);
RT_API int rt_rec_classes(const rt_session* s);
/* "<det arch>/<det dtype> <cls dtype> <rec arch>/<rec dtype>", e.g. "mobile/f32 f32 mobile/f32" or "server/f16 f16 server/f16":
 * which graphs the model sources held and the arithmetic they run in (library-owned string) */
RT_API const char* rt_model_info(const rt_session* s);

/* ---- stage functions (host buffers; computed on the GPU) ------------------------- */
RT_API int rt_resize_both_dims(const rt_session* s, int h, int w, int* out_h, int* out_w);
RT_API int rt_resize_both(rt_session* s, const uint8_t* rgb, int h, int w, uint8_t* out, int out_h, int out_w);
RT_API int rt_det_input_dims(const rt_session* s, int h, int w, int* out_h, int* out_w);
/* a3: u8 HWC RGB (after resize_both) -> f32 [1,3,out_h,out_w] */
RT_API int rt_det_preprocess(rt_session* s, const uint8_t* rgb, int h, int w, float* out_nchw);
/* a5: f32 [h,w] map -> boxes (n x 8 f32: TL,TR,BR,BL x,y in ori_* coordinates) + scores. */
RT_API int rt_det_postprocess(rt_session* s, const float* pred, int h, int w, int ori_h, int ori_w,
                              float* boxes, float* scores, int max_out, int* n_out);
/* a6: crop sizes for n boxes (w,h after the optional rotate270), then the crops packed
 * back to back (RGB8) into out (capacity out_cap bytes). */
RT_API int rt_crop_dims(const float* boxes, int n, int* ws, int* hs);
RT_API int rt_crop_images(rt_session* s, const uint8_t* rgb, int h, int w, const float* boxes, int n,
                          uint8_t* out, size_t out_cap);
/* rt_crop_images with the launch form chosen: form 0 = one grid row per crop, each as long as the largest crop (what
 * rt_crop_images and crop_source = Resized run), form 1 = the flat list of output pixels (crop_source = Original,
 * rt_run_regions).  Both run the same per-pixel code: the outputs are equal byte for byte. */
RT_API int rt_debug_warp_crops(rt_session* s, const uint8_t* rgb, int h, int w, const float* boxes, int n, int form,
                               uint8_t* out, size_t out_cap);
RT_API int rt_scale_and_clip(float* boxes, int n, double bitmap_w, double bitmap_h, double ori_w, double ori_h);
/* a8/a10: one crop -> f32 [3,img_h,W]; W = img_w when max_wh_ratio <= 0 else (int)(img_h*max_wh_ratio). */
RT_API int rt_resize_norm_width(int img_h, int img_w, float max_wh_ratio);
RT_API int rt_resize_norm_image(rt_session* s, const uint8_t* crop, int h, int w, int ori_h, int ori_w,
                                int img_h, int img_w, float max_wh_ratio, float* out_chw);
/* a12: probs [n,T,C] -> argmax idx [n,T], max prob [n,T], kept tokens [n,T] (+count), score [n] */
RT_API int rt_ctc_decode(rt_session* s, const float* probs, int n, int t, int c, int32_t* idx, float* prob,
                         int32_t* tokens, int32_t* n_tokens, float* scores);

/* ---- L2: RettoSession::run over a batch of pages --------------------------------- */
#define RT_MEM_HOST 0
#define RT_MEM_DEVICE 1
#define RT_MEM_HOST_MAPS_DEVICE 2   /* pages in host memory (what RettoSession::run is handed, session.rs:108-131), override maps in HBM */
/* rgb[i]: RGB8 HWC page i (hs[i] x ws[i]); mem says where the pixels live.
 * det_map_override (may be NULL, entries may be NULL): f32 [H,W] probability map at the
 * det input size of page i, in the memory space of the pages (RT_MEM_HOST_MAPS_DEVICE: in
 * device memory beside host pages), used INSTEAD of the det network's output when building
 * boxes (the network still runs).  This is the hook the synthetic-weights benchmark and the
 * teacher-forced parity tests use; a deployment has no such maps, so a host-fed measurement
 * keeps them in HBM and sends only the pages over PCIe. */
RT_API int rt_run_batch(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages,
                        int mem, const float* const* det_map_override, rt_results** out);
/* RettoSession::run_stream (session.rs:133-143): as rt_run_batch, and cb(user, page, stage, json) is called for
 * every page with the stage's RettoWorkerStageResult JSON (stage 0 = Det, 1 = Cls, 2 = Rec; the reference's
 * mpsc::Sender order Det -> Cls -> Rec per image is kept).  Det is delivered as soon as the boxes of the page
 * are known -- before its crops are classified or read; Cls and Rec when the call completes.  Callbacks come
 * from the library's lane threads, one at a time; json is only valid during the call. */
typedef void (*rt_stage_callback)(void* user, int page, int stage, const char* json);
RT_API int rt_run_batch_stream(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages,
                               int mem, const float* const* det_map_override, rt_stage_callback cb, void* user,
                               rt_results** out);
/* Asynchronous form of rt_run_batch (round 4) -- the counterpart of RettoSession::run_stream's worker thread + channel
 * (session.rs:108-143): rt_submit_batch splits the pages over the session's lanes exactly as rt_run_batch does and returns at
 * once; rt_wait_batch blocks until that batch is complete and returns its results (same object, same order, same values as
 * rt_run_batch).  Up to RT_MAX_INFLIGHT batches may be submitted ahead: a lane works through its parts of consecutive batches
 * back to back, so the host-side result assembly of batch i and the first kernels of batch i + 1 overlap with the other lanes'
 * work.  The argument ARRAYS are copied by rt_submit_batch; the PAGES (and override maps) they point to must stay valid and
 * unchanged until rt_wait_batch has returned for that ticket.  Every ticket must be waited for exactly once (any order); until
 * then every other call on the session except rt_submit_batch / rt_wait_batch fails with RT_ERR_INVALID.  rt_wait_batch of a
 * failed batch returns the failing stage's status (the other batches in flight are not affected).
 * Host pages (RT_MEM_HOST, RT_MEM_HOST_MAPS_DEVICE) are copied to HBM by rt_submit_batch itself, on a copy stream of the session,
 * part by part right before each lane's job is queued: with a batch submitted ahead the transfer of batch i + 1 runs under the
 * kernels of batch i, and no lane waits for PCIe with an empty stream.  The session keeps one staging buffer per batch in flight
 * (the batch's page bytes; reused).  From pageable memory the copy has completed when rt_submit_batch returns; from pinned memory
 * it is asynchronous -- either way the rule above (pages unchanged until rt_wait_batch) is the contract. */
#define RT_MAX_INFLIGHT 8   /* (a cap on queued tickets only: a lane works on one part at a time, whatever is queued behind it) */
typedef struct rt_ticket rt_ticket;
RT_API int rt_submit_batch(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                           const float* const* det_map_override, rt_ticket** out);
RT_API int rt_wait_batch(rt_session* s, rt_ticket* ticket, rt_results** out);
/* Det tiles (retto_amd/csrc/det_tiles.h states the rule): large pages detected at their own resolution.  A caller who raises
 * max_side_len (or det_limit_side_len) so that a 7680 x 4320 scan reaches the detector unshrunk would otherwise push one image
 * of 33 Mpixel through the det network: every activation resident at once, squeeze-excite pooled over the whole scan, every
 * layer at a shape nobody tuned.  With tiles on, a page whose det input is larger than `tile` in either direction is run through
 * the det network as overlapping tiles of tile x tile pixels (a direction the page fits into keeps its length), and each tile's
 * trusted part -- up to the middle of the overlap with its neighbour -- is copied into the ONE page probability map.  The copy
 * is a selection, every page pixel comes from exactly one tile; DB post-processing, the boxes, the crops, cls, rec and every rec
 * option run on that map unchanged, rt_results_det_checksum is taken over it, a det_map_override still has the page's det
 * size.  The tiles of all pages of a call share the det launch groups (and rt_config.det_sub_batch) with the untiled pages.
 * A page that fits into one tile takes the whole-page path bit for bit, and with tiles off (the default) nothing is launched
 * that was not before.  rt_run_regions and rt_det never tile.
 * tile = 0: off; otherwise a multiple of 32, at least 64.  overlap: a multiple of 32, 0 <= overlap <= tile / 2 (64 suits the
 * default det graph).  Anything else: RT_ERR_INVALID naming the parameter.  The setting holds for the pipeline calls that follow
 * on every lane (rt_submit_* takes it as it is at the call); fails like every other call while tickets are in flight.
 * The largest det input, tiled or not, is RT_DET_MAX_PIXELS pixels (DB post-processing indexes a page's pixels, rows and hull
 * points with int; 8192 x 32736, say): a page beyond it fails with RT_ERR_CAPACITY before anything is queued.
 * rt_config.max_boxes_per_page stays the caller's knob for pages with many lines. */
#define RT_DET_MAX_PIXELS 268434432
RT_API int rt_set_det_tiles(rt_session* s, int tile, int overlap);
/* the setting (each optional); RT_ERR_INVALID for a NULL session */
RT_API int rt_det_tiles(const rt_session* s, int* tile, int* overlap);
/* The tile plan of a det input of h x w (both multiples of 32), GPU-free and sessionless.  *n_rows x *n_cols tiles of *tile_h x
 * *tile_w pixels, in row-major order; tile row i starts at row_origin[i] and owns the page rows [i ? row_bound[i - 1] : 0,
 * row_bound[i]), likewise the columns.  Each output is optional; arrays are written when row_cap / col_cap hold the plan
 * (RT_ERR_INVALID otherwise, the counts still written).  A page that is not tiled (tile = 0, or it fits) is one tile.  Bad
 * parameters: RT_ERR_INVALID naming the parameter; more than RT_DET_MAX_PIXELS: RT_ERR_CAPACITY (rt_last_error(NULL)). */
RT_API int rt_det_tile_plan(int h, int w, int tile, int overlap, int32_t* row_origin, int32_t* row_bound, int row_cap,
                            int32_t* col_origin, int32_t* col_bound, int col_cap, int* n_rows, int* n_cols, int* tile_h, int* tile_w);
/* The det stage of a one-page pipeline call on rgb_det, a host RGB8 image at det-input size h x w, under the session's det tiles:
 * the pipeline's own function and launch groups.  tile_maps_out (optional): every tile's own map, tile_h x tile_w floats each,
 * packed in plan order; page_map_out [h * w]: the stitched map (the network's map for a page that is not tiled). */
RT_API int rt_debug_det_tiles(rt_session* s, const uint8_t* rgb_det, int h, int w, float* tile_maps_out, float* page_map_out);
/* Rec windows (retto_amd/csrc/rec_windows.h states the rule): long lines read at a familiar width.  Det tiles and crop_source = 1
 * produce long lines: a text line across a 7680-pixel scan is a 48 x 3000 rec tensor with 400 time steps, which the recogniser
 * would read as one image -- its attention over all 400 steps, every squeeze-excite block pooled over the whole line.  With
 * windows on, a rec line at least 8 columns wider than `window` is run through the rec network as overlapping units of `window`
 * columns (the last one up to 7 wider), and each unit's trusted time steps -- up to the middle of the overlap with its neighbour
 * -- are copied into the ONE line's rows of per-step (index, probability) and head-input features.  The copy is a selection,
 * every time step comes from exactly one unit; the line keeps its number of time steps and its geometry, so the greedy decode,
 * word boxes, candidates, charsets, lexicons and snap, patterns, keywords and beams run on it unchanged.  The units of all lines
 * of a rec launch group run in one pass of the network.  A line that is not windowed takes the whole-line path, a group without
 * a windowed line launches nothing that it did not before, and with windows off (the default) nothing changes.  It applies to
 * every pipeline entry point, rt_run_regions* included; rt_rec, rt_rec_ragged and rt_ctc_decode never window.
 * window = 0: off; otherwise a multiple of 32, at least 128.  overlap: a multiple of 32, 0 <= overlap <= window / 2.  Anything
 * else: RT_ERR_INVALID naming the parameter.  The setting holds for the pipeline calls that follow on every lane (rt_submit_*
 * takes it as it is at the call); fails like every other call while tickets are in flight.
 * What windows do to accuracy with trained PP-OCRv4 weights has NOT been measured; a multiple of the 320 base width is the
 * familiar regime, nothing more is recommended. */
RT_API int rt_set_rec_windows(rt_session* s, int window, int overlap);
/* the setting (each optional); RT_ERR_INVALID for a NULL session */
RT_API int rt_rec_windows(const rt_session* s, int* window, int* overlap);
/* The window plan of a rec line of L >= 8 columns, GPU-free and sessionless.  *n units, *T = the line's time steps; unit i covers
 * the columns [origin[i], origin[i] + width[i]), its time step k is the line's step origin[i] / 8 + k, and it owns the line's
 * steps [i ? bound[i - 1] : 0, bound[i]).  Each output is optional; the arrays are written when cap holds the plan
 * (RT_ERR_INVALID otherwise, the counts still written).  A line that is not windowed (window = 0, or L < window + 8) is one
 * unit.  Bad parameters: RT_ERR_INVALID naming the parameter (rt_last_error(NULL)). */
RT_API int rt_rec_window_plan(int L, int window, int overlap, int32_t* origin, int32_t* width, int32_t* bound, int cap, int* n, int* T);
/* the number of units line `line` of page `page` was read in: 1 for a whole line, 0 out of range */
RT_API int rt_results_rec_windows(const rt_results* r, int page, int line);
/* n lines of [3, 48, widths[i]] (host, NCHW, concatenated, as rt_rec_ragged takes them) run as ONE rec group through the
 * pipeline's own cut, network and stitch functions under the session's rec windows.  Every output is optional: every unit's rows
 * in unit order, line after line (unit_idx_out / unit_prob_out: one per unit time step; unit_z5_out: 120 floats per step), and
 * the stitched rows of every line (line_*_out, likewise, one row per line time step). */
RT_API int rt_debug_rec_windows(rt_session* s, const float* nchw, int n, const int* widths, int32_t* unit_idx_out,
                                float* unit_prob_out, float* unit_z5_out, int32_t* line_idx_out, float* line_prob_out,
                                float* line_z5_out);
/* Rec flip (retto_amd/csrc/rec_flip.h states the rule): lines the angle classifier is unsure of are read both ways up, and the
 * better reading is kept.  Whether a line is upside down is otherwise decided by the small classifier and the fixed cls_thresh
 * alone: a line labelled 180 at score 0.7 is not rotated, a line wrongly labelled 0 stays upside down, and rt_run_regions*
 * callers hand in quads in any corner order -- and an upside-down line is garbage for every rec option.  With cls_below > 0 a
 * line whose classifier score (rt_results_cls_scores) is below cls_below (fp32 <) is run through the recogniser as it is (view
 * 0) and rotated by 180 degrees (view 1: the rotated crop through the same resize_norm at the same width), both in the one pass
 * of its rec launch group; each view gets the greedy CTC score (kept probabilities summed in step order over the kept count),
 * and view 1 is taken iff it kept a token and view 0 kept none or score1 > score0 (a tie or a NaN keeps view 0).  The chosen
 * view's per-step rows become the line's rows by copy, so the greedy decode, charsets, lexicons and snap, patterns, keywords,
 * beams, word boxes, candidates and windows run on the chosen reading; word boxes and keyword quads take (classifier rotated)
 * XOR (view 1 taken) as their rotation.  rt_results_cls_labels / _cls_scores stay the classifier's own outputs.
 * cls_below = 0: off (the default); any value above 1 reads every line both ways; NaN, a negative value or an infinity:
 * RT_ERR_INVALID naming the parameter.  The setting holds for the pipeline calls that follow on every lane (rt_submit_* takes it
 * as it is at the call), rt_run_regions* and the encoded entry points included; rt_rec, rt_rec_ragged and rt_ctc_decode never
 * flip; fails like every other call while tickets are in flight.
 * Cost: a both-ways line costs the rec network twice (it is charged twice in its launch group's pixel budget), plus two small
 * copy kernels per group with such a line.  With 0 < cls_below <= 1 every call SYNCS ITS LANE ONCE MORE, between the classifier
 * and the rec plan, to bring one float per line to the host; above 1 there is no extra sync.  A group without a both-ways line,
 * and every call with flip off, launch and allocate nothing new.
 * Not supported: a per-region flag, 90 / 270 degree views, switching the classifier off, a choice by anything but the greedy
 * score.  What flipping does to accuracy with trained PP-OCRv4 weights has NOT been measured (the weights here are synthetic). */
RT_API int rt_set_rec_flip(rt_session* s, float cls_below);
/* the setting (optional); RT_ERR_INVALID for a NULL session */
RT_API int rt_rec_flip(const rt_session* s, float* cls_below);
/* The rule of the choice, GPU-free and sessionless: 1 when view 1 is taken given the two views' kept tokens and greedy scores */
RT_API int rt_rec_flip_choose(int ntok0, float score0, int ntok1, float score1);
/* line `line` of page `page`: 0 when it was read one way or is out of range (the scores are then untouched), 1 when it was read
 * both ways and view 0 was kept, 2 when view 1 was taken; score0 / score1 (each optional): the views' greedy scores (NaN for a
 * view that kept no token) */
RT_API int rt_results_rec_flip(const rt_results* r, int page, int line, float* score0, float* score1);
/* n RGB8 crops packed back to back in host memory (crop i is hw[2 i] rows of hw[2 i + 1] pixels) run as ONE rec group through the
 * pipeline's own rotate, resize_norm, network, score and select functions under the session's rec windows, every line at the
 * padded width of max_wh_ratio with T time steps.  both[i] != 0: line i is read both ways.  The views are the n lines' view 0 in
 * line order, then the flagged lines' view 1 in line order.  Every output is optional: per view its rows (view_idx_out /
 * view_prob_out [views][T], view_z5_out [views][T][120]), kept tokens and greedy score ([views]); taken_out [n]: 1 where view 1 was taken; the lines' final
 * rows idx_out / prob_out [n][T] and z5_out [n][T][120].  NULL or bad arguments (n <= 0, an empty crop, a ratio that is not
 * positive and finite): RT_ERR_INVALID before any device work. */
RT_API int rt_debug_rec_flip(rt_session* s, const uint8_t* crops, const int32_t* hw, int n, const uint8_t* both, float max_wh_ratio,
                             int32_t* view_idx_out, float* view_prob_out, float* view_z5_out, int32_t* view_ntok_out,
                             float* view_score_out, int32_t* taken_out, int32_t* idx_out, float* prob_out, float* z5_out);
/* The pipeline over regions the caller already knows (form fields, subtitles, corrected boxes, another detector's boxes):
 * quads[i] = n_quads[i] x 8 floats in host memory, TL, TR, BR, BL of each region in original-page coordinates; mem
 * (RT_MEM_HOST or RT_MEM_DEVICE) says where the pages live.  Every coordinate is clamped to [0, ori - 1] (no rounding); line k
 * of page i is get_crop_img(page i, clamped quad k), cut from the page as handed in, whatever rt_config.crop_source says.
 * resize_both, the det network and DB post-processing do not run; the crop plan, the flat warp, cls, the rec plan, rec and
 * CTC (word boxes and candidates when configured) are the pipeline's own stages.  Pages are split over the lanes as by
 * rt_run_batch.  The results object is rt_run_batch's: lines keep the caller's order, rt_results_boxes returns the clamped
 * quads, rt_results_det_scores is 1.0f for every line, rt_results_det_checksum is 0.
 * RT_ERR_INVALID, with a message naming the page and the region, and nothing queued: a non-finite coordinate, a clamped quad
 * whose crop is less than one pixel wide or high, a singular homography, a negative count, NULL quads[i] with n_quads[i] > 0.
 * Fails like every other call while tickets are in flight.  A crop of more than 2^31 - 1 pixels is RT_ERR_IMAGE, here and in
 * every other call that plans crops (its pixel count used to overflow the plan's 32-bit arithmetic). */
RT_API int rt_run_regions(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                          const float* const* quads, const int* n_quads, rt_results** out);
RT_API void rt_results_free(rt_results* r);
RT_API int rt_results_pages(const rt_results* r);
RT_API int rt_results_count(const rt_results* r, int page);
/* det: boxes in ORIGINAL image coordinates (session.rs:94-97) */
RT_API const float* rt_results_boxes(const rt_results* r, int page);      /* n x 8 */
RT_API const float* rt_results_det_scores(const rt_results* r, int page); /* n */
RT_API const uint16_t* rt_results_cls_labels(const rt_results* r, int page);
RT_API const float* rt_results_cls_scores(const rt_results* r, int page);
RT_API const float* rt_results_rec_scores(const rt_results* r, int page);
RT_API int rt_results_rec_tokens(const rt_results* r, int page, int line, const int32_t** tokens);
RT_API const char* rt_results_rec_text(const rt_results* r, int page, int line); /* UTF-8 */
/* ---- word boxes (rt_config.rec_return_word_box = 1) ------------------------------------------------------------------------
 * The words of each line, from the time steps of its kept CTC tokens.  The rule is this library's own (the reference has none);
 * retto_amd/csrc/word_boxes.h states it, and k_word_boxes runs it on the device right after the CTC decode.  In short:
 *   - each dictionary entry gets a raw class: DIGIT (all ASCII 0-9), ALPHA (ASCII [A-Za-z0-9], not DIGIT), DOT ".", HYPHEN "-",
 *     CJK (every code point in U+4E00-U+9FFF), SPLIT (anything else, the appended " " included);
 *   - kept tokens become ALNUM (ALPHA, DIGIT; "-" after ALNUM; "." between ALNUM and a DIGIT), CJK or SPLIT;
 *   - every CJK token is a word (kind 0), every maximal run of ALNUM tokens is a word (kind 1), SPLIT tokens belong to none;
 *   - an ALNUM word spans its columns [c_first, c_last + 1) times the crop pixels per column; a CJK word is centred on its
 *     column with the mean CJK pitch of the line as its width; spans are clamped to the crop, y covers the whole crop;
 *   - the span is mapped back through the cls rotate180, the crop's rotate270 and the crop homography to the page, then
 *     scale_and_clip'd like the line boxes.  quad: TL, TR, BR, BL in the line box's corner order.
 * Differences from PaddleOCR's return_word_box: no pixel parity with cal_ocr_word_box is intended; the spans go through the
 * crop's homography (rotated boxes and crops map correctly) instead of an axis-aligned offset, and CJK / ALNUM splitting is by
 * the classes above.  first_token / n_tokens index rt_results_rec_tokens of the line; first_col / last_col are time steps. */
typedef struct rt_word {
  float quad[8];
  int32_t first_token, n_tokens, first_col, last_col, kind;   /* kind: 0 CJK character, 1 alphanumeric run */
} rt_word;
/* number of words of the line (0 when the option is off); *words: library-owned, valid until rt_results_free */
RT_API int rt_results_rec_words(const rt_results* r, int page, int line, const rt_word** words);
/* UTF-8 text of one word: the dictionary entries of its tokens, joined (NULL when out of range) */
RT_API const char* rt_results_rec_word_text(rt_results* r, int page, int line, int word);
/* The word rule on the CPU, GPU-free and sessionless.  dict: dictionary file bytes (parsed as rt_parse_dictionary does);
 * tokens / cols: n kept class ids and their time steps (cols strictly increasing, < T); T, W, resized_w: the line's rec
 * tensor (tokens_for_width(W) steps, padded width W, resized width); box8_after: the line's det box in after-resize_both
 * coordinates, from which the crop's size, rotate270 and homography are derived exactly as the pipeline does; rot180: the
 * cls rotation was applied.  out: room for n words; *n_words their number.  Quads in original-image coordinates. */
RT_API int rt_debug_word_boxes(const void* dict, size_t dict_len, const int32_t* tokens, const int32_t* cols, int n, int T, int W,
                               int resized_w, const float* box8_after, int rot180, int after_w, int after_h, int ori_w, int ori_h,
                               rt_word* out, int* n_words);
/* ---- token candidates (rt_config.rec_return_candidates = K) ------------------------------------------------------------------
 * Per kept CTC token of a line: its time step and K (class id, probability) pairs.  retto_amd/csrc/ctc_candidates.h states the
 * rule; in short, for token j kept at time step cols[j]:
 *   - rank 0 is the decode's own choice: (token id, the fused CTC head's probability at that step), bit for bit what the line's
 *     rec score averages;
 *   - ranks 1 .. K-1 are the other classes (the blank 0 included) with the largest logits, recomputed in fp32 from the head's
 *     input features for the kept rows only, ordered by logit descending, then id ascending; their probabilities are the softmax
 *     over every class of the recomputed logits;
 *   - (-1, 0.0f) fills the row when the model has fewer than K classes.
 * Near ties: the recomputed logits come from another GEMM launch than the fused head's, so a runner-up's probability may exceed
 * rank 0's by rounding; rank 0 stays the decode's choice.  K = 1 recomputes nothing (confidences and time steps only).  Ranks
 * >= 1 are repeatable run to run and equal across rt_run_batch, submit / wait and the encoded entry points on the same batch;
 * they are NOT promised bit-identical when the batch around a line changes (the logits GEMM's plan may depend on the number of
 * kept rows).  Everything else the session returns is bit-identical to K = 0. */
typedef struct rt_candidate { int32_t id; float prob; } rt_candidate;
/* returns K (0 when the option is off or page / line are out of range).  *cands: [n_tokens][K] row-major, *cols: [n_tokens],
 * n_tokens = what rt_results_rec_tokens returns for the line; either pointer may be NULL.  Library-owned until rt_results_free. */
RT_API int rt_results_rec_candidates(const rt_results* r, int page, int line, const rt_candidate** cands, const int32_t** cols);
/* The device path of the option on host arrays (k_ctc_kept_rows, row gather, the CTC FC GEMM, k_ctc_topk; chunk_rows kept rows
 * per GEMM, 0 = the production chunk).  z5 [rows][120]: head input features; W [120][N], bias [N] (or NULL): the CTC FC; idx /
 * prob [rows]: the fused head's argmax and probability per time step; tokens_per_line [n_lines]: time steps per line (sum =
 * rows).  Kept token j of a line whose first row is o: cols_out[o + j], cands_out[(o + j) * K .. + K); entries past a line's
 * token count keep what the caller put there.  n_tokens_out [n_lines]: kept tokens per line.  z5 may be NULL when K = 1. */
RT_API int rt_debug_ctc_candidates(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* idx,
                                   const float* prob, const int32_t* tokens_per_line, int n_lines, int K, int chunk_rows,
                                   rt_candidate* cands_out, int32_t* cols_out, int32_t* n_tokens_out);
/* The same rule on the CPU in plain fp32 loops (ctc_candidates.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_candidates_host(const float* z5, const float* W, const float* bias, int N, const int32_t* idx,
                                        const float* prob, const int32_t* tokens_per_line, int n_lines, int K,
                                        rt_candidate* cands_out, int32_t* cols_out, int32_t* n_tokens_out);
/* ---- rec charsets: a line's CTC decode restricted to the characters the caller allows ---------------------------------------
 * For callers who know what a region can hold (digits in a form field, Latin capitals on a plate).  Filtering tokens afterwards
 * cannot bring back a runner-up that WAS allowed, and rec_return_candidates only covers the time steps the unrestricted decode
 * kept; a charset changes the decode itself.  retto_amd/csrc/ctc_charset.h states the rule; in short, for every time step of a
 * line that carries charset S (a set of class ids that always holds the blank 0):
 *   - the logits of the step are recomputed in fp32 from the head's input features, as for candidates;
 *   - the step's class is the one of S with the largest logit (ties to the lower id), its probability the softmax over S only;
 *   - these replace the fused head's values before the greedy decode: the keep rule, the line score, word boxes, candidates and
 *     JSON run unchanged over them.  With rec_return_candidates = K ranks >= 1 name classes of S only, with probabilities over
 *     S; (-1, 0.0f) fills the row when S has fewer than K classes.
 * Lines without a charset, and every det / cls result, are bit-identical to a session that never created one.  The reference
 * has no counterpart.  Results of a restricted line are repeatable run to run and equal across the entry points on one batch
 * (ctc_charset.h says why, under today's GEMM plan, they do not depend on the rest of the batch either).
 *
 * rt_charset_create: S = the blank, every dictionary class whose WHOLE entry is one code point of utf8 [len bytes] (duplicate
 * entries all join; U+0020 selects the appended " " class; a multi-code-point entry can only be named through ids), and ids
 * [n_ids] (class ids, may be NULL with n_ids = 0).  *charset_out: the new id, 1-based, valid until rt_destroy; a session holds at
 * most RT_MAX_CHARSETS.  Errors: a code point that matches no entry -> RT_ERR_INVALID naming it as U+XXXX; malformed UTF-8 ->
 * RT_ERR_UTF8; an id outside [0, classes) -> RT_ERR_INVALID; the cap -> RT_ERR_CAPACITY.  Fails like every other call while
 * tickets are in flight. */
#define RT_MAX_CHARSETS 64
RT_API int rt_charset_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, int n_ids, int* charset_out);
/* |S| of a charset (0 for an unknown id); *ids (optional): its class ids in ascending order, library-owned until rt_destroy */
RT_API int rt_charset_classes(const rt_session* s, int charset, const int32_t** ids);
/* The session default: the charset of every line of every pipeline call that follows (rt_run_batch, _stream, rt_submit_batch,
 * the encoded entry points, rt_run_regions); 0 = none (the initial state).  rt_submit_* takes the value as it is at the call. */
RT_API int rt_set_rec_charset(rt_session* s, int charset);
/* rt_run_regions with a charset per region: charsets[i][k] for region k of page i; -1 = the session default, 0 = unrestricted,
 * >= 1 = that charset.  charsets == NULL or charsets[i] == NULL: -1 throughout.  An unknown id: RT_ERR_INVALID naming the page
 * and the region, nothing queued. */
RT_API int rt_run_regions_charsets(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                                   const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                                   rt_results** out);
/* What rt_charset_create compiles, GPU-free and sessionless: dict = dictionary file bytes (parsed as rt_parse_dictionary does);
 * mask_out [mask_cap >= ceil(classes / 32)]: class c is bit (c & 31) of word c >> 5; *n_classes: the dictionary's class count.
 * The same code, errors and messages as rt_charset_create (err: optional, err_cap bytes). */
RT_API int rt_debug_charset_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, const int32_t* ids, int n_ids,
                                    uint32_t* mask_out, int mask_cap, int* n_classes, char* err, size_t err_cap);
/* The device path of the charsets on host arrays (row gather, the CTC FC GEMM, k_ctc_charset_argmax; then the greedy decode
 * and, with K > 0, the candidates path with the masks).  z5, W, bias, N, tokens_per_line, n_lines, K (0 .. RT_MAX_CANDIDATES),
 * chunk_rows, cands_out, cols_out: as rt_debug_ctc_candidates (cands_out / cols_out may be NULL when K = 0).  line_set
 * [n_lines]: 0 = none, s >= 1 = the set at masks[(s - 1) * ceil(N / 32) ...]; masks [n_sets][ceil(N / 32)] (the blank is allowed
 * whatever bit 0 says).  idx / prob [rows] are in-out: the rows of restricted lines are replaced, the others come back untouched.
 * tokens_out [rows]: line i's tokens from its first row on (entries past its count keep what the caller put there);
 * n_tokens_out, scores_out [n_lines]: the decode's counts and scores (NaN for a line without tokens). */
RT_API int rt_debug_ctc_charset(rt_session* s, const float* z5, const float* W, const float* bias, int N, int32_t* idx, float* prob,
                                const int32_t* tokens_per_line, int n_lines, const int32_t* line_set, const uint32_t* masks,
                                int n_sets, int K, int chunk_rows, int32_t* tokens_out, int32_t* n_tokens_out, float* scores_out,
                                rt_candidate* cands_out, int32_t* cols_out);
/* The same rule on the CPU in plain fp32 loops (ctc_charset.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_charset_host(const float* z5, const float* W, const float* bias, int N, int32_t* idx, float* prob,
                                     const int32_t* tokens_per_line, int n_lines, const int32_t* line_set, const uint32_t* masks,
                                     int n_sets, int K, int32_t* tokens_out, int32_t* n_tokens_out, float* scores_out,
                                     rt_candidate* cands_out, int32_t* cols_out);
/* ---- rec lexicons: a caller's word list ranked by CTC likelihood per line -----------------------------------------------------
 * For the enumerated field: the region holds one of N known strings (a country, a product code, a station name).  A charset only
 * narrows the alphabet, candidates only exist at the time steps the greedy decode kept, and matching the greedy text against the
 * list afterwards throws the model's probabilities away.  retto_amd/csrc/ctc_lexicon.h states the rule; in short, for a line of T
 * time steps that carries a lexicon:
 *   - the logits of every step are recomputed in fp32 from the head's input features, as for candidates and charsets, and turned
 *     into log-probabilities by the FULL softmax over every class (a charset on the same line does not change them);
 *   - every entry's CTC forward log-likelihood is computed in the log domain in fp32; an entry that cannot fit into T steps
 *     (T < its length + its number of equal neighbours) is infeasible and never reported;
 *   - the line reports up to RT_LEXICON_MATCHES feasible entries, by loglik descending then entry index ascending, each with
 *     posterior = exp(loglik - log-sum-exp over the line's feasible entries).
 * One limit: the lexicon lines that one rec group takes (about 24 M crop pixels) may carry 2^26 entries between them (1024 lines
 * of a 65536-entry lexicon); a call past it fails with RT_ERR_CAPACITY.
 * The line's tokens, score, text, word boxes, candidates and JSON stay what they are without the lexicon, bit for bit, unless the
 * caller switches the lexicon's snap on (rt_lexicon_set_snap below).  Lines without a lexicon cost nothing.  The reference has no
 * counterpart.
 *
 * rt_lexicon_create: the entries are the lines of utf8 [len bytes] (split and trimmed as rt_parse_dictionary's lines; empty
 * lines skipped), read code point by code point, each the LOWEST class id whose whole dictionary entry is that code point (U+0020
 * is the appended " "); then n_id_entries entries given as class ids, entry_lens[i] ids each, consecutive in ids (may be NULL
 * with n_id_entries = 0).  Entry numbers count from 0 in that order.  *lexicon_out: the new id, 1-based, valid until rt_destroy;
 * a session holds at most RT_MAX_LEXICONS.  Errors: a code point that matches no entry -> RT_ERR_INVALID naming it as U+XXXX and
 * the entry; malformed UTF-8 -> RT_ERR_UTF8; an id of 0 or outside [1, classes), an empty id entry, an entry of more than
 * RT_LEXICON_MAX_LEN ids, no entry at all -> RT_ERR_INVALID; more than RT_LEXICON_MAX_ENTRIES entries, or the lexicon cap ->
 * RT_ERR_CAPACITY.  Fails like every other call while tickets are in flight. */
#define RT_MAX_LEXICONS 16
#define RT_LEXICON_MAX_ENTRIES 65536
#define RT_LEXICON_MAX_LEN 31
#define RT_LEXICON_MATCHES 4
typedef struct rt_lexicon_match { int32_t entry; float loglik; float posterior; } rt_lexicon_match;
RT_API int rt_lexicon_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens,
                             int n_id_entries, int* lexicon_out);
/* the number of entries of a lexicon (0 for an unknown id) */
RT_API int rt_lexicon_entries(const rt_session* s, int lexicon);
/* the length of an entry (0 for an unknown lexicon or entry); *ids (optional): its class ids, library-owned until rt_destroy */
RT_API int rt_lexicon_entry(const rt_session* s, int lexicon, int entry, const int32_t** ids);
/* an entry as UTF-8 (its classes' dictionary texts joined), library-owned until rt_destroy; NULL for an unknown lexicon or entry */
RT_API const char* rt_lexicon_entry_text(const rt_session* s, int lexicon, int entry);
/* The session default: the lexicon of every line of every pipeline call that follows; 0 = none (the initial state).
 * rt_submit_* takes the value as it is at the call. */
RT_API int rt_set_rec_lexicon(rt_session* s, int lexicon);
/* rt_run_regions with a charset and a lexicon per region: charsets[i][k] / lexicons[i][k] for region k of page i; -1 = the
 * session default, 0 = none, >= 1 = that charset / lexicon.  Either array, or an entry of it, may be NULL: -1 throughout.  An
 * unknown id: RT_ERR_INVALID naming the page and the region, nothing queued. */
RT_API int rt_run_regions_lexicons(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                                   const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                                   const int32_t* const* lexicons, rt_results** out);
/* the matches of a line: their number (0 when the line had no lexicon); *m (optional): the matches, best first */
RT_API int rt_results_rec_lexicon(const rt_results* r, int page, int line, const rt_lexicon_match** m);
/* the lexicon a line was scored against (0: none) */
RT_API int rt_results_rec_lexicon_id(const rt_results* r, int page, int line);
/* Lexicon snap: replace a line's decode by its aligned best entry (retto_amd/csrc/ctc_lexicon_align.h states the rule).  Off by
 * default, switched on per lexicon: a line that carries the lexicon snaps iff min_posterior > 0, the line has at least one match
 * and matches[0].posterior >= min_posterior (an fp32 comparison; a NaN never snaps).  Match 0 -- the forward winner -- is then
 * aligned to the line's time steps by a CTC Viterbi pass on the GPU (raw logits, fp32, ties to the earlier state: alignments
 * pack to the left) and the path replaces the line's per-step (class, probability) rows before the CTC decode: the line's
 * tokens are the entry's ids, its text the entry's text, a token's time step the first frame of its run, its probability the
 * FULL softmax's at that frame, the score their mean; word boxes, candidates (rank 0 is that pair; ranks >= 1 as without snap)
 * and the JSON follow from the same rows.  With a charset on the same line the charset decodes first and a snap that fires
 * replaces its rows; where it does not fire the charset's decode stands.  A line that does not snap, a line of a lexicon with
 * min_posterior = 0 and a line without a lexicon are bit-identical to a call without snap, and the rt_lexicon_match lists are
 * the same for every line.  With no lexicon that has snap on, nothing new is launched or allocated.
 * Out of scope: snapping on rt_rec and rt_ctc_decode, a per-region threshold, sharing the logits with the charset pass, and
 * aligning entries other than match 0.
 * rt_lexicon_set_snap: min_posterior in [0, 1], 0 = never snap (the initial state); an unknown lexicon id, a NaN or a value
 * outside [0, 1] -> RT_ERR_INVALID.  May be changed between calls; fails like rt_lexicon_create while tickets are in flight. */
RT_API int rt_lexicon_set_snap(rt_session* s, int lexicon, float min_posterior);
/* a lexicon's current min_posterior (0 for an unknown id) */
RT_API float rt_lexicon_snap(const rt_session* s, int lexicon);
/* 1 where the line's decode is its aligned best entry, else 0 (also for out-of-range arguments, a line with no lexicon, NULL) */
RT_API int rt_results_rec_lexicon_snapped(const rt_results* r, int page, int line);
/* What rt_lexicon_create compiles, GPU-free and sessionless: dict = dictionary file bytes (parsed as rt_parse_dictionary does).
 * ids_out [ids_cap] / lens_out [lens_cap]: the entries' class ids, entry after entry, and their lengths; *n_ids_out / *n_entries_out:
 * how many there are (also when a cap was too small: RT_ERR_INVALID then, nothing copied); *n_classes: the dictionary's class
 * count.  The same code, errors and messages as rt_lexicon_create (err: optional, err_cap bytes). */
RT_API int rt_debug_lexicon_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, const int32_t* ids,
                                    const int32_t* entry_lens, int n_id_entries, int32_t* ids_out, int ids_cap, int32_t* lens_out,
                                    int lens_cap, int* n_ids_out, int* n_entries_out, int* n_classes, char* err, size_t err_cap);
/* The device path of the lexicons on host arrays (row gather in chunks of whole lines, the CTC FC GEMM, k_ctc_row_lse,
 * k_ctc_lexicon_forward, k_ctc_lexicon_topk).  z5, W, bias, N, tokens_per_line, n_lines, chunk_rows: as rt_debug_ctc_charset.
 * line_lex [n_lines]: 0 = none, k >= 1 = lexicon k, whose entries are [lex_first_entry[k - 1], lex_first_entry[k]) of the flat
 * list: entry j has entry_lens[j] ids (1 .. RT_LEXICON_MAX_LEN, each in [1, N)), consecutive in entry_ids; lex_first_entry
 * [n_lex + 1] ascends from 0, every lexicon has at least one entry.  loglik_out (optional): the full table, line after line, one
 * float per entry of the line's lexicon (none for a line of lexicon 0), -inf where infeasible.  matches_out [n_lines]
 * [RT_LEXICON_MATCHES], n_matches_out [n_lines]: slots past a line's count, and everything of a line of lexicon 0 but its count
 * (0), keep what the caller put there. */
RT_API int rt_debug_ctc_lexicon(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                const int32_t* tokens_per_line, int n_lines, const int32_t* line_lex, const int32_t* entry_ids,
                                const int32_t* entry_lens, const int32_t* lex_first_entry, int n_lex, int chunk_rows,
                                float* loglik_out, rt_lexicon_match* matches_out, int32_t* n_matches_out);
/* The same rule on the CPU in plain fp32 loops (ctc_lexicon.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_lexicon_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                     int n_lines, const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                                     const int32_t* lex_first_entry, int n_lex, float* loglik_out, rt_lexicon_match* matches_out,
                                     int32_t* n_matches_out);
/* The device path of the lexicon snap on host arrays: rt_debug_ctc_lexicon's, with k_ctc_lexicon_topk per chunk and
 * k_ctc_lexicon_align behind it.  rt_debug_ctc_lexicon's arguments, and lex_min_post [n_lex]: each lexicon's min_posterior, in
 * [0, 1]; idx [rows] / prob [rows], in and out: the lines' per-step rows, overwritten by the aligned path for the lines that
 * snap -- rows of every other line come back untouched; snapped_out [n_lines]: 0 / 1 for every line of a lexicon, the caller's
 * value kept for lines of lexicon 0; vit_out [n_lines]: the end state's fp32 Viterbi value in the raw-logit domain, written for
 * snapped lines only.  loglik_out, matches_out, n_matches_out: exactly what rt_debug_ctc_lexicon returns. */
RT_API int rt_debug_ctc_lexicon_align(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                      const int32_t* tokens_per_line, int n_lines, const int32_t* line_lex, const int32_t* entry_ids,
                                      const int32_t* entry_lens, const int32_t* lex_first_entry, int n_lex, const float* lex_min_post,
                                      int chunk_rows, int32_t* idx, float* prob, int32_t* snapped_out, float* vit_out,
                                      float* loglik_out, rt_lexicon_match* matches_out, int32_t* n_matches_out);
/* The same rule on the CPU in plain fp32 loops (ctc_lexicon_align.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_lexicon_align_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                           int n_lines, const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                                           const int32_t* lex_first_entry, int n_lex, const float* lex_min_post, int32_t* idx,
                                           float* prob, int32_t* snapped_out, float* vit_out, float* loglik_out,
                                           rt_lexicon_match* matches_out, int32_t* n_matches_out);
/* ---- rec patterns (retto_amd/csrc/ctc_pattern.h): a line's CTC decode constrained to a regular expression ----
 * The pattern language, the compiled form (a trimmed DFA over class groups), the Viterbi rule and its tie order are stated in that
 * header.  For the field whose format is known ("[0-9]{4}-[0-9]{2}-[0-9]{2}"): a line that carries a pattern decodes to the best
 * CTC path whose collapsed string the pattern accepts -- text, tokens, time steps, score, word boxes, candidates (rank 0 = the
 * path's (id, prob)) and JSON all follow, as for a lexicon snap.  A line too short for the pattern (T < min_steps) is unmatched
 * and keeps its decode (its charset's, if it has one: the charset writes first).  Lines without a pattern are bit-identical to a
 * run without patterns.  A line may not carry both a pattern and a lexicon: RT_ERR_INVALID naming the page and the region (for
 * the session defaults: at the call), nothing queued.
 * RT_PATTERN_MAX_STATES counts the states of the automaton as built (subset construction of the position automaton, dead states
 * removed, NOT minimised: "[ab]*" has two states); RT_PATTERN_MAX_PAIRS counts the (state entered, class) pairs.  Either limit, or
 * repeats that write out to more than 4096 atoms, gives RT_ERR_CAPACITY; a wide set (".{8}" over a large dictionary) belongs
 * into a charset. */
#define RT_MAX_PATTERNS 16
#define RT_PATTERN_MAX_STATES 64
#define RT_PATTERN_MAX_PAIRS 4096
#define RT_PATTERN_MAX_BYTES 1024
typedef struct rt_pattern_result { int32_t pattern, matched; float logprob, free_logprob; } rt_pattern_result;
/* compiles utf8 [len] over the session's dictionary; *pattern_out = its 1-based id, valid until rt_destroy.  RT_ERR_UTF8 /
 * RT_ERR_INVALID / RT_ERR_CAPACITY with a message naming the byte offset.  Fails while tickets are in flight. */
RT_API int rt_pattern_create(rt_session* s, const char* utf8, size_t len, int* pattern_out);
/* a pattern's states, pairs and the fewest time steps a line needs to match it (each optional); RT_ERR_INVALID for an unknown id */
RT_API int rt_pattern_info(const rt_session* s, int pattern, int* states, int* pairs, int* min_steps);
/* the pattern's text as given (NULL for an unknown id); library-owned */
RT_API const char* rt_pattern_text(const rt_session* s, int pattern);
/* the pattern of every line of the pipeline calls that follow (rt_submit_* takes it as it is at the call); 0 = none */
RT_API int rt_set_rec_pattern(rt_session* s, int pattern);
/* rt_run_regions_lexicons with one pattern id per region as well: -1 = the session default, 0 = none, >= 1 = that pattern; each
 * of the three arrays, and each page's entry, may be NULL */
RT_API int rt_run_regions_patterns(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                                   const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                                   const int32_t* const* lexicons, const int32_t* const* patterns, rt_results** out);
/* 1 where the line carried a pattern (*out, optional: which, whether it matched, the path's log-probability and the unconstrained
 * best path's: logprob - free_logprob <= 0 is what the format cost; an unmatched line reports logprob = -inf), else 0 */
RT_API int rt_results_rec_pattern(const rt_results* r, int page, int line, rt_pattern_result* out);
/* The pattern compiler, GPU-free and sessionless: dict = dictionary file bytes (parsed as rt_parse_dictionary does), utf8 [len]
 * the pattern.  group_of_out [group_cap >= classes], delta_out [delta_cap >= S * G] (-1: no arc), accept_out [accept_cap >= S];
 * *S_out, *G_out, *P_out, *min_steps_out, *n_classes are written also when a cap was too small (RT_ERR_INVALID then, nothing
 * copied).  RT_ERR_UTF8 / RT_ERR_INVALID / RT_ERR_CAPACITY with a message naming the byte offset (err: optional, err_cap bytes). */
RT_API int rt_debug_pattern_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, int32_t* group_of_out,
                                    int group_cap, int32_t* delta_out, int delta_cap, int32_t* accept_out, int accept_cap, int* S_out,
                                    int* G_out, int* P_out, int* min_steps_out, int* n_classes, char* err, size_t err_cap);
/* The device path of the patterns on host arrays (row gather in chunks of whole lines, the CTC FC GEMM, k_ctc_row_lse,
 * k_ctc_row_max, k_ctc_pattern_viterbi).  z5, W, bias, N, tokens_per_line, n_lines, chunk_rows: as rt_debug_ctc_lexicon_align.
 * line_pat [n_lines]: 0 = none, k >= 1 = pattern k of the n_pat given as flat compiled tables: pat_S [n_pat], pat_G [n_pat],
 * group_of [n_pat][N], and pattern k's delta [S][G] and accept [S] behind pattern k - 1's -- so it runs at any N without a
 * dictionary.  idx [rows] / prob [rows], in and out: overwritten by the path for the matched lines, rows of every other line come
 * back untouched.  matched_out / vit_out / logprob_out / free_out [n_lines]: written for every line of a pattern (an unmatched
 * one: 0, -inf, -inf and its free_logprob), the caller's values kept for lines of pattern 0. */
RT_API int rt_debug_ctc_pattern(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                const int32_t* tokens_per_line, int n_lines, const int32_t* line_pat, const int32_t* pat_S,
                                const int32_t* pat_G, const int32_t* group_of, const int32_t* delta, const int32_t* accept, int n_pat,
                                int chunk_rows, int32_t* idx, float* prob, int32_t* matched_out, float* vit_out, float* logprob_out,
                                float* free_out);
/* The same rule on the CPU in plain fp32 loops (ctc_pattern.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_pattern_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                     int n_lines, const int32_t* line_pat, const int32_t* pat_S, const int32_t* pat_G,
                                     const int32_t* group_of, const int32_t* delta, const int32_t* accept, int n_pat, int32_t* idx,
                                     float* prob, int32_t* matched_out, float* vit_out, float* logprob_out, float* free_out);

/* ---- rec keywords: a caller's keyword list spotted inside every line ----------------------------------------------------------
 * For the page-level question "where does it say Total, Invoice No, this customer's name".  A lexicon ranks whole lines only, a
 * pattern .*Total.* over the whole dictionary passes RT_PATTERN_MAX_PAIRS, and searching the decoded text afterwards loses the
 * hit to one weak frame.  retto_amd/csrc/ctc_keyword.h states the rule; in short, for a line of T time steps that carries a list
 * and each entry of the list:
 *   score      the log-ratio of the best CTC path whose collapsed string CONTAINS the entry as a substring over the best
 *              unconstrained path, from the line's recomputed fp32 logits; <= 0, and exactly 0 where the greedy path holds it;
 *   span       first_col, last_col: the time steps that best occurrence covers (ties: the earliest start, then the earliest end);
 *   hits       the entries that fit the line (T >= length + equal neighbours) with score >= the list's min_score, up to
 *              RT_KEYWORD_HITS of them, by score descending, then entry number ascending;
 *   quad       the span [first_col, last_col + 1) on the page, mapped exactly as a word of rt_config.rec_return_word_box is (it
 *              needs no option: the quads are computed on the host for lines with hits only).
 * One occurrence per (line, entry): the best.  Several occurrences, length normalisation and whole-word matching are out of scope.
 * Keywords only read a line: they go with any charset, lexicon or pattern, and every other result -- boxes, tokens, text, scores,
 * words, candidates, lexicon matches and snaps, pattern results, JSON -- is what it is without them, bit for bit.  The per-stage
 * JSON stays as it is: keyword hits are not serialised.  With no list created nothing new is launched or allocated.  One limit,
 * as for lexicons: the keyword lines one rec group takes may carry 2^26 entries between them; past it RT_ERR_CAPACITY.
 *
 * rt_keywords_create: rt_lexicon_create's arguments, errors and messages (the entries go through the same compiler; at most
 * RT_LEXICON_MAX_ENTRIES entries of at most RT_LEXICON_MAX_LEN ids), and min_score <= 0, fixed for the list's life: -INFINITY
 * reports the best hits whatever they score, 0 only exact-zero hits; a NaN or a value above 0 -> RT_ERR_INVALID; more than
 * RT_MAX_KEYWORD_LISTS lists -> RT_ERR_CAPACITY.  *list_out: the new id, 1-based, valid until rt_destroy.  Fails like
 * rt_lexicon_create while tickets are in flight. */
#define RT_MAX_KEYWORD_LISTS 16
#define RT_KEYWORD_HITS 8
typedef struct rt_keyword_hit { int32_t entry; float score; int32_t first_col, last_col; float quad[8]; } rt_keyword_hit;
RT_API int rt_keywords_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens,
                              int n_id_entries, float min_score, int* list_out);
/* rt_lexicon_entries / _entry / _entry_text for a keyword list; rt_keywords_min_score: NaN for an unknown id */
RT_API int rt_keywords_entries(const rt_session* s, int list);
RT_API int rt_keywords_entry(const rt_session* s, int list, int entry, const int32_t** ids);
RT_API const char* rt_keywords_entry_text(const rt_session* s, int list, int entry);
RT_API float rt_keywords_min_score(const rt_session* s, int list);
/* The session default: the keyword list of every line of every pipeline call that follows; 0 = none (the initial state). */
RT_API int rt_set_rec_keywords(rt_session* s, int list);
/* rt_run_regions_patterns with one keyword list id per region as well: -1 = the session default, 0 = none, >= 1 = that list;
 * each array, or an entry of it, may be NULL: -1 throughout.  An unknown id -> RT_ERR_INVALID naming page and region; the
 * keywords of a page are checked behind its charsets, lexicons and patterns. */
RT_API int rt_run_regions_keywords(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                                   const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                                   const int32_t* const* lexicons, const int32_t* const* patterns,
                                   const int32_t* const* keywords, rt_results** out);
/* the hits of a line: their number (0 when the line had no list); *hits (optional): the hits, best first */
RT_API int rt_results_rec_keywords(const rt_results* r, int page, int line, const rt_keyword_hit** hits);
/* the keyword list a line was searched for (0: none) */
RT_API int rt_results_rec_keywords_id(const rt_results* r, int page, int line);
/* The device path of the keywords on host arrays (row gather in chunks of whole lines, the CTC FC GEMM, k_ctc_row_max,
 * k_ctc_keyword_spot, k_ctc_keyword_topk).  z5, W, bias, N, tokens_per_line, n_lines, chunk_rows: as rt_debug_ctc_lexicon.
 * line_kw [n_lines]: 0 = none, k >= 1 = list k, whose entries are [kw_first_entry[k - 1], kw_first_entry[k]) of the flat entry
 * list entry_lens, their ids consecutive in entry_ids; kw_first_entry [n_kw + 1] ascends from 0, every list has at least one
 * entry; kw_min_score [n_kw]: each list's min_score.  score_out, span_out [.][2] (both optional): the full tables, line after
 * line, one score and one (first_col, last_col) per entry of the line's list (none for a line of list 0); -inf and (-1, -1) where
 * infeasible.  hits_out [n_lines][RT_KEYWORD_HITS], n_hits_out [n_lines]: slots past a line's count, every hit's quad, and
 * everything of a line of list 0 but its count of 0, come back as the caller put them. */
RT_API int rt_debug_ctc_keywords(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                 const int32_t* tokens_per_line, int n_lines, const int32_t* line_kw, const int32_t* entry_ids,
                                 const int32_t* entry_lens, const int32_t* kw_first_entry, int n_kw, const float* kw_min_score,
                                 int chunk_rows, float* score_out, int32_t* span_out, rt_keyword_hit* hits_out, int32_t* n_hits_out);
/* The same rule on the CPU in plain fp32 loops (ctc_keyword.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_keywords_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                      int n_lines, const int32_t* line_kw, const int32_t* entry_ids, const int32_t* entry_lens,
                                      const int32_t* kw_first_entry, int n_kw, const float* kw_min_score, float* score_out,
                                      int32_t* span_out, rt_keyword_hit* hits_out, int32_t* n_hits_out);
/* Host-only: the page quad of the span [first_col, last_col + 1) of a line, from rt_debug_word_boxes' geometry arguments (T, W,
 * resized_w, the line's det box after resize_both, rot180, the page's sizes) -> quad8_out in original-image coordinates: what
 * rt_results_rec_keywords reports for a hit with that span. */
RT_API int rt_debug_span_quad(int T, int W, int resized_w, const float* box8_after, int rot180, int after_w, int after_h, int ori_w,
                              int ori_h, int first_col, int last_col, float* quad8_out);

/* ---- rec beams: the N most probable strings of a line by CTC prefix beam search ------------------------------------------------
 * The greedy decode is the best PATH; rec_return_candidates gives alternatives at the steps it kept; a lexicon ranks a given
 * list; patterns and keywords are Viterbi searches.  A spell corrector, a language model or a validator that takes the first
 * hypothesis that parses asks for the most probable STRINGS, each summed over its alignments, and how far apart they are.
 * retto_amd/csrc/ctc_beam.h states the rule; in short, for a line of T time steps, beam width B and N hypotheses:
 *   hypothesis  a string with the log-probabilities of its alignments that end in the blank (pb) and in a non-blank (pnb), from
 *               the line's recomputed fp32 logits under the FULL softmax (a charset of the line is not applied);
 *   step        every member stays (blank, or its last class again) and is extended by each of the step's 8 best non-blank
 *               classes; an extension that IS another member's string is added to that member, never kept twice; the best B by
 *               total log-probability survive (ties: stays before extensions, then beam order, then the class's rank);
 *   result      the first N of the final beam, best first: tokens and logprob.  The empty string is a legitimate hypothesis with
 *               0 tokens; fewer than N where the beam is smaller; none for a line without time steps.
 * logprob sums the alignments that stayed inside the beam: never more than the string's full CTC likelihood, equal to it where
 * the beam never overflowed.  Beams only read a line: they go with every charset, lexicon, pattern and keyword list, and every
 * other result -- boxes, tokens, text, scores, words, candidates, matches, hits, JSON -- is what it is without them, bit for bit.
 * The per-stage JSON stays as it is.  Off (the default): no launch, no workspace.
 *
 * rt_set_rec_beam: beam = 0 switches the option off; otherwise 1 <= beam <= RT_MAX_BEAM and 1 <= nbest <= min(beam, RT_MAX_NBEST),
 * else RT_ERR_INVALID.  It applies to every pipeline call that follows, rt_run_regions* included; it fails like the other
 * setters while tickets are in flight.  rt_rec_beam reads the two values back. */
#define RT_MAX_BEAM 32
#define RT_MAX_NBEST 8
typedef struct rt_beam { float logprob; int32_t n_tokens; } rt_beam;
RT_API int rt_set_rec_beam(rt_session* s, int beam, int nbest);
RT_API int rt_rec_beam(const rt_session* s, int* beam, int* nbest);
/* the hypotheses of a line: their number (0 when the option was off); *out (optional): their records, best first */
RT_API int rt_results_rec_beams(const rt_results* r, int page, int line, const rt_beam** out);
/* hypothesis k of a line: its number of tokens; *tokens (optional): its class ids in reading order */
RT_API int rt_results_rec_beam_tokens(const rt_results* r, int page, int line, int k, const int32_t** tokens);
/* hypothesis k of a line as UTF-8, built from the dictionary as rt_results_rec_text is (NULL for a k the line does not have) */
RT_API const char* rt_results_rec_beam_text(const rt_results* r, int page, int line, int k);
/* The device path of the beams on host arrays (row gather in chunks of whole lines, the CTC FC GEMM, k_ctc_row_lse,
 * k_ctc_beam_topc, k_ctc_beam_search): every line carries the beam.  z5, W, bias, N, tokens_per_line, n_lines, chunk_rows: as
 * rt_debug_ctc_keywords.  counts_out [n_lines]; beams_out [n_lines][nbest]; tokens_out: line after line [nbest][T], hypothesis k
 * of a line at its k * T.  Record slots past a line's count and token slots past a hypothesis' n_tokens come back as the caller
 * put them.  beam = 0 or n_lines = 0: nothing runs and nothing is written. */
RT_API int rt_debug_ctc_beam(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                             int n_lines, int beam, int nbest, int chunk_rows, int32_t* counts_out, rt_beam* beams_out,
                             int32_t* tokens_out);
/* The same rule on the CPU in plain fp32 loops (ctc_beam.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_beam_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                  int n_lines, int beam, int nbest, int32_t* counts_out, rt_beam* beams_out, int32_t* tokens_out);

/* ---- rec language model: a character n-gram fused into the beam search -----------------------------------------------------------
 * The standard companion of a CTC prefix beam search.  Re-ranking the N-best list afterwards is not the same thing: a string that
 * was pruned at step t cannot come back, so the model acts inside every step's selection.  retto_amd/csrc/ctc_lm.h states the
 * rule; in short:
 *   model    a back-off n-gram over the recogniser's classes, order 1 .. RT_MAX_LM_ORDER, at most RT_MAX_LM_NGRAMS n-grams, given
 *            as ARPA text ("\data\", "ngram k=count", "\k-grams:" sections of "log10 p <tab> tokens [<tab> log10 backoff]",
 *            "\end\").  A token is the UTF-8 text of one dictionary entry, "<sp>" the entry that is U+0020, "<s>" the line start.
 *            An n-gram with "</s>" or with a token the dictionary lacks is dropped and counted; "<unk>"'s unigram, if present,
 *            gives the out-of-vocabulary log-probability, else oov_log10 does (finite, at most 0);
 *   lm       of a string: the sum over its tokens, in reading order from the start state, of the model's log-probability (natural
 *            log, fp32) of the token after its context, backing off as ARPA models do; 0 for the empty string;
 *   fused    score = logprob + (alpha * lm + beta * n_tokens); alpha >= 0, both finite;
 *   step     the beam's rule with one change: the best B candidates are the best by fused score (ties as before).
 * rt_beam.logprob stays the CTC total, never above the string's full likelihood; the hypotheses come in fused order.  Everything
 * else of a call -- and, with no model attached, the hypotheses too -- is what it is without it, bit for bit; the per-stage JSON
 * stays as it is.  What the model does to accuracy with the real PP-OCRv4 weights has not been measured.
 *
 * rt_lm_create: compiles arpa [len] over the session's dictionary and puts its tables on the device; *lm_out = its handle, 0-based,
 * valid until rt_destroy; a session holds at most RT_MAX_LMS.  RT_ERR_INVALID with a message that names the line for a number that
 * is not finite, an n-gram that is there twice, an n-gram whose context (its first k - 1 tokens) is not an n-gram, an order above
 * RT_MAX_LM_ORDER, more than RT_MAX_LM_NGRAMS kept n-grams, a malformed line or a file without its end mark; RT_ERR_CAPACITY past
 * RT_MAX_LMS.  Fails like every other call while tickets are in flight.
 * rt_lm_info: the model's order, its kept and dropped n-grams and its states (each optional); RT_ERR_INVALID for an unknown handle.
 * rt_set_rec_beam_lm: lm = -1 switches fusion off; otherwise a handle, alpha >= 0 and both weights finite, else RT_ERR_INVALID.
 * Legal while beam = 0, and without effect until rt_set_rec_beam sets one; it applies to every pipeline call that follows and
 * fails like the other setters while tickets are in flight.  rt_rec_beam_lm reads the three values back (each optional). */
#define RT_MAX_LM_ORDER 5
#define RT_MAX_LM_NGRAMS (1 << 22)
#define RT_MAX_LMS 4
typedef struct rt_beam_lm { float lm; float score; } rt_beam_lm;
RT_API int rt_lm_create(rt_session* s, const char* arpa, size_t len, float oov_log10, int* lm_out);
RT_API int rt_lm_info(const rt_session* s, int lm, int* order, int* ngrams, int* dropped, int* states);
RT_API int rt_set_rec_beam_lm(rt_session* s, int lm, float alpha, float beta);
RT_API int rt_rec_beam_lm(const rt_session* s, int* lm, float* alpha, float* beta);
/* the lm and fused score of a line's hypotheses, beside rt_results_rec_beams' records: their number, and 0 with nothing written
 * when fusion was off; *out (optional): the records, best first */
RT_API int rt_results_rec_beam_lm(const rt_results* r, int page, int line, const rt_beam_lm** out);
/* The ARPA compiler without a session: dict [dict_len] as rt_config.dict, arpa [len], oov_log10 -> the id form: n-gram i has
 * ngram_lens_out[i] ids, one n-gram after the other in ngram_ids_out (<s> = *n_classes), with logp_out[i] and backoff_out[i] as
 * NATURAL logs.  *n_out, *n_ids_out: how many n-grams and ids there are (also when a cap was too small: RT_ERR_INVALID then,
 * nothing copied); *order_out, *dropped_out, *states_out: as rt_lm_info; *oov_out: the out-of-vocabulary log-probability, natural. */
RT_API int rt_debug_lm_compile(const void* dict, size_t dict_len, const char* arpa, size_t len, float oov_log10, int32_t* ngram_ids_out,
                               int ids_cap, int32_t* ngram_lens_out, float* logp_out, float* backoff_out, int n_cap, int* n_ids_out,
                               int* n_out, int* order_out, int* dropped_out, int* states_out, float* oov_out, int* n_classes,
                               char* err, size_t err_cap);
/* A model in its id form over `classes` classes (oov: natural log) compiled and walked on the host: string i has string_lens[i]
 * ids of [1, classes), one string after the other in strings; lm_out[i]: its lm; state_out[i]: the state it ends in (0: the empty
 * context; k + 1: the k-th n-gram of the id form among those shorter than the order).  Refusals as rt_lm_create's, naming the
 * n-gram's index. */
RT_API int rt_debug_lm_score(int classes, const int32_t* ngram_ids, const int32_t* ngram_lens, const float* logp, const float* backoff,
                             int n, float oov, const int32_t* strings, const int32_t* string_lens, int n_strings, float* lm_out,
                             int32_t* state_out, char* err, size_t err_cap);
/* rt_debug_ctc_beam with a model in its id form over the head's N classes and the weights: the device path with
 * k_ctc_beam_search's fused variant.  lm_out [n_lines][nbest] beside beams_out; slots past a line's count come back as the caller
 * put them.  A bad model or weight is refused before any launch. */
RT_API int rt_debug_ctc_beam_lm(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                int n_lines, int beam, int nbest, int chunk_rows, const int32_t* ngram_ids, const int32_t* ngram_lens,
                                const float* logp, const float* backoff, int n, float oov, float alpha, float beta,
                                int32_t* counts_out, rt_beam* beams_out, int32_t* tokens_out, rt_beam_lm* lm_out);
/* The same rule on the CPU in plain fp32 loops (ctc_beam.h, ctc_lm.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_beam_lm_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                     int n_lines, int beam, int nbest, const int32_t* ngram_ids, const int32_t* ngram_lens,
                                     const float* logp, const float* backoff, int n, float oov, float alpha, float beta,
                                     int32_t* counts_out, rt_beam* beams_out, int32_t* tokens_out, rt_beam_lm* lm_out);

/* ---- rec vocabulary: a word-list constraint fused into the beam search ------------------------------------------------------------
 * "This is running text, and its words should be words of this list": a language's word list, a product catalogue, a customer's
 * field vocabulary.  A character n-gram cannot tell `recieve` from `receive`, a lexicon ranks whole lines, and re-ranking the
 * N-best list afterwards cannot bring back a string that was pruned on the way, so the list acts inside every step's selection,
 * beside the language model where one is attached.  retto_amd/csrc/ctc_vocab.h states the rule; in short:
 *   words      1 .. RT_VOCAB_MAX_LEN class ids each, at most RT_VOCAB_MAX_WORDS; a word given twice is one word;
 *   classes    the classes that occur in some word are WORD classes; every other class (digits, punctuation, the space, as far
 *              as the list does not spell with them) is a SEPARATOR: it passes freely and ends a word;
 *   oov_words  of a string: its maximal runs of word classes that are not words of the list.  While the search runs, a last run
 *              still open counts only once it is no prefix of a word any more; the line end closes it;
 *   score      logprob (with a model: rt_beam_lm.score) - gamma * oov_words; gamma >= 0, finite;
 *   step       the beam's rule with one change: the best B candidates are the best by that score over the count so far (ties as
 *              before); after the last step the final beam is ranked once more by the score over the closed count.
 * The constraint is soft: a line is never left without hypotheses.  rt_beam.logprob stays the CTC total and rt_beam_lm what it
 * is (its score holds no gamma).  gamma = 0 gives the bytes of the search without a vocabulary.  Everything else of a call --
 * and, with no vocabulary attached, the hypotheses too -- is what it is without it, bit for bit; the per-stage JSON stays as it
 * is.  What the option does to accuracy with the real PP-OCRv4 weights has not been measured.
 *
 * rt_vocab_create: the words are the lines of utf8 [len] (may be NULL with len 0), split, trimmed and mapped code point by code
 * point to the lowest class exactly as rt_lexicon_create maps its entries, then n_id_words words of word_lens[i] ids each,
 * consecutive in ids.  flags & RT_VOCAB_CASE_VARIANTS: every UTF-8 word is also inserted with its first ASCII letter upper-cased
 * and with all its ASCII letters upper-cased; a variant with a code point the dictionary lacks is not inserted, and is counted.
 * *vocab_out = its handle, 0-based, valid until rt_destroy; a session holds at most RT_MAX_VOCABS.  RT_ERR_UTF8 for malformed
 * text; RT_ERR_INVALID with a message that names the word for a code point that matches no dictionary entry ("U+XXXX"), the
 * blank or an id outside [1, classes), an empty or over-long word, no word at all, unknown flag bits; RT_ERR_CAPACITY past
 * RT_VOCAB_MAX_WORDS or RT_MAX_VOCABS.  Fails like every other call while tickets are in flight.
 * rt_vocab_info: the vocabulary's words, trie nodes (the root included), word classes and dropped case variants (each
 * optional); RT_ERR_INVALID for an unknown handle.
 * rt_set_rec_beam_vocab: vocab = -1 switches the constraint off; otherwise a handle and gamma >= 0, finite, else RT_ERR_INVALID.
 * Legal while beam = 0, and without effect until rt_set_rec_beam sets one; it applies to every pipeline call that follows and
 * fails like the other setters while tickets are in flight.  rt_rec_beam_vocab reads the two values back (each optional). */
#define RT_VOCAB_MAX_LEN 63
#define RT_VOCAB_MAX_WORDS (1 << 20)
#define RT_MAX_VOCABS 4
#define RT_VOCAB_CASE_VARIANTS 1
typedef struct rt_beam_vocab { int32_t oov_words; float score; } rt_beam_vocab;
RT_API int rt_vocab_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens, int n_id_words,
                           int flags, int* vocab_out);
RT_API int rt_vocab_info(const rt_session* s, int vocab, int* words, int* nodes, int* word_classes, int* variants_dropped);
RT_API int rt_set_rec_beam_vocab(rt_session* s, int vocab, float gamma);
RT_API int rt_rec_beam_vocab(const rt_session* s, int* vocab, float* gamma);
/* the closed count and the score of a line's hypotheses, beside rt_results_rec_beams' records: their number, and 0 with nothing
 * written when no vocabulary was attached; *out (optional): the records, best first */
RT_API int rt_results_rec_beam_vocab(const rt_results* r, int page, int line, const rt_beam_vocab** out);
/* The vocabulary compiler without a session: dict [dict_len] as rt_config.dict, utf8 [len], flags -> the id form: word i has
 * word_lens_out[i] ids, one word after the other in word_ids_out, each word once, in order of first occurrence.  *n_out,
 * *n_ids_out: how many words and ids there are (also when a cap was too small: RT_ERR_INVALID then, nothing copied); *words_out,
 * *nodes_out, *word_classes_out, *variants_dropped_out: as rt_vocab_info. */
RT_API int rt_debug_vocab_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, int flags, int32_t* word_ids_out,
                                  int ids_cap, int32_t* word_lens_out, int n_cap, int* n_ids_out, int* n_out, int* words_out,
                                  int* nodes_out, int* word_classes_out, int* variants_dropped_out, int* n_classes, char* err,
                                  size_t err_cap);
/* A vocabulary in its id form over `classes` classes compiled and walked on the host: string i has string_lens[i] ids of
 * [1, classes), one string after the other in strings; open_out[i]: the count while the string's last word is open, closed_out[i]:
 * the count with the line end, state_out[i]: the trie node it ends in (0: the root; -1: inside a word that left the trie).
 * Refusals as rt_vocab_create's, naming the word's index. */
RT_API int rt_debug_vocab_walk(int classes, const int32_t* word_ids, const int32_t* word_lens, int n_words, const int32_t* strings,
                               const int32_t* string_lens, int n_strings, int32_t* open_out, int32_t* closed_out, int32_t* state_out,
                               char* err, size_t err_cap);
/* rt_debug_ctc_beam_lm with a vocabulary in its id form over the head's N classes and gamma: the device path with
 * k_ctc_beam_search's vocabulary variants.  n = 0 n-grams with alpha = beta = 0 means no model, and lm_out may be NULL then.
 * vocab_out [n_lines][nbest] beside beams_out; slots past a line's count come back as the caller put them.  Anything bad is
 * refused before any launch. */
RT_API int rt_debug_ctc_beam_vocab(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                   int n_lines, int beam, int nbest, int chunk_rows, const int32_t* ngram_ids, const int32_t* ngram_lens,
                                   const float* logp, const float* backoff, int n, float oov, float alpha, float beta,
                                   const int32_t* word_ids, const int32_t* word_lens, int n_words, float gamma, int32_t* counts_out,
                                   rt_beam* beams_out, int32_t* tokens_out, rt_beam_lm* lm_out, rt_beam_vocab* vocab_out);
/* The same rule on the CPU in plain fp32 loops (ctc_beam.h, ctc_lm.h, ctc_vocab.h), GPU-free and sessionless; same layout. */
RT_API int rt_debug_ctc_beam_vocab_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                        int n_lines, int beam, int nbest, const int32_t* ngram_ids, const int32_t* ngram_lens,
                                        const float* logp, const float* backoff, int n, float oov, float alpha, float beta,
                                        const int32_t* word_ids, const int32_t* word_lens, int n_words, float gamma,
                                        int32_t* counts_out, rt_beam* beams_out, int32_t* tokens_out, rt_beam_lm* lm_out,
                                        rt_beam_vocab* vocab_out);
/* f32 sum of every det probability map produced in the call (keeps the network's
 * output observable when det_map_override is used) */
RT_API double rt_results_det_checksum(const rt_results* r);
/* RettoWorkerStageResult JSON of one page in the serde shape retto-wasm emits
 * (retto-wasm/fe/index.ts:5-42); stage 0 = det, 1 = cls, 2 = rec. Library-owned. */
RT_API const char* rt_results_json(rt_results* r, int page, int stage);

/* ---- device memory + timing helpers for harnesses -------------------------------- */
RT_API int rt_device_malloc(rt_session* s, size_t bytes, void** out);
RT_API int rt_device_free(rt_session* s, void* p);
RT_API int rt_memcpy_h2d(rt_session* s, void* dst, const void* src, size_t bytes);
RT_API int rt_memcpy_d2h(rt_session* s, void* dst, const void* src, size_t bytes);
RT_API int rt_synchronize(rt_session* s);
/* Per-kernel-family device time of the last rt_run_batch / L1 call, measured with HIP
 * events on the session's own stream.  names/ms are library-owned arrays of *n entries. */
/* Upper bound on the concurrent lanes rt_run_batch uses from now on (<= the number created by
 * rt_config.lanes).  1 = strictly serial on the session's own stream (what the per-kernel
 * profile wants: concurrent lanes share the GPU and stretch each other's kernels). */
RT_API int rt_set_lanes(rt_session* s, int lanes);
/* on: 0 off; 1 every launch family ("gemm_pw/...", "dwconv5", ...) and the enclosing network scopes ("net/det", "net/cls",
 * "net/rec"); 2 the network scopes only (the per-launch event pairs are themselves work on the stream: whole-network device
 * times are read from a pass without them). */
RT_API int rt_profile_enable(rt_session* s, int on);
RT_API int rt_profile_get(rt_session* s, const char* const** names, const float** ms, const int** calls, int* n);

/* ---- model files -----------------------------------------------------
 * Replaces the model loading of retto-core/src/worker/ort_worker.rs:120-135 (the .onnx bytes
 * resolved by worker.rs:30-56 go to ONNX Runtime there).  rt_config's det / cls / rec sources
 * may hold either an RTWB blob or the PP-OCRv4 .onnx file itself: non-RTWB bytes are imported
 * by rt_create through the same code as rt_onnx_to_rtwb.  which: 0 det, 1 cls, 2 rec.
 * Host-only (no GPU needed).  *out is library-owned until rt_buffer_free; on failure err
 * (optional, err_cap bytes) receives the message and the RT_ERR_* code is returned. */
RT_API int rt_onnx_to_rtwb(int which, const void* onnx, size_t len, void** out, size_t* out_len, char* err, size_t err_cap);
RT_API void rt_buffer_free(void* p);

/* ---- encoded pages ----------------------------------------------------
 * rt_decode_image replaces ImageHelper::new_from_raw_img_flow (retto-core/src/image_helper.rs:34-44:
 * image::load_from_memory(bytes)?.to_rgb8()): PNG (all colour types / depths, Adam7), Huffman
 * JPEG (sequential and progressive; grey / YCbCr, any sampling), PNM, uncompressed BMP -> tightly packed RGB8 [h][w][3],
 * alpha dropped, 16-bit samples as (v + 128) / 257.  Host-only.  *rgb is library-owned until
 * rt_buffer_free.  Unknown / corrupt input: RT_ERR_IMAGE with the reason in err (optional).
 * rt_run_encoded_batch is RettoSession::run / run_stream (session.rs:108-143) over encoded
 * bytes: pages are decoded on host threads, then processed as by rt_run_batch_stream (cb may be NULL). */
/* Host CPUs this process should plan with: the affinity mask capped by the cgroup CPU quota, divided by LOCAL_WORLD_SIZE (one
 * process per GPU on a node).  rt_run_encoded_batch sizes its decode-thread pool with it (at most 16); std::thread::
 * hardware_concurrency() would report the machine (256 on the MI355X box) to a pod that owns 16 CPUs.  No reference counterpart
 * (retto-cli decodes on the calling thread, retto-cli/src/main.rs:80-86). */
RT_API int rt_host_cpu_budget(void);
RT_API int rt_decode_image(const void* data, size_t len, uint8_t** rgb, int* h, int* w, char* err, size_t err_cap);
RT_API int rt_run_encoded_batch(rt_session* s, const void* const* files, const size_t* lens, int n_pages,
                                rt_stage_callback cb, void* user, rt_results** out);
/* Encoded pages with the pixel work on the GPU.  The host only entropy-decodes each JPEG page (on the thread pool of
 * rt_run_encoded_batch) into quantised int16 coefficients; dequantisation, the inverse DCT, chroma upsampling and colour
 * conversion run on the device, bit-identical to rt_decode_image.  A JPEG page goes to the device when every coefficient fits
 * int16 and its sampling is grey, 4:4:4, 4:2:2 or 4:2:0 (each chroma factor 1x1, 2x1 or 2x2); every other page -- other JPEG
 * layouts, PNG, PNM, BMP -- is decoded on the host as rt_decode_image does and its pixels are uploaded.  Decode errors are
 * rt_decode_image's (RT_ERR_IMAGE, "image decode: ..."), reported for the first failing page in page order.
 *
 * rt_submit_encoded_batch is rt_submit_batch over encoded files: the pages are decoded inside the call, the returned ticket
 * is collected with rt_wait_batch and gives what rt_run_encoded_batch gives for the same files.  Unlike rt_submit_batch's
 * pages, the FILE BUFFERS may be freed as soon as the call returns: the ticket owns the coefficients.  Each lane part's upload
 * and reconstruction run on the session's copy stream before that lane starts, so the host decode of batch i + 1 (inside this
 * call) overlaps the GPU work of batch i.  On a decode error nothing is queued, *out is NULL and tickets in flight are not
 * affected.  Legal wherever rt_submit_batch is.
 *
 * rt_decode_batch decodes n files synchronously through the same host stage and kernels.  out == NULL: hs / ws only, from the
 * headers (no pixel work, the rest of a file is not checked).  Otherwise out[i] receives hs[i] * ws[i] * 3 bytes of RGB8 in
 * `mem` (RT_MEM_HOST or RT_MEM_DEVICE); on_device (optional) [i] = 1 where the kernels reconstructed page i.  Fails with
 * RT_ERR_INVALID while tickets are in flight, like every call other than rt_submit_batch / rt_wait_batch.
 *
 * rt_debug_jpeg_reconstruct: one file through the same host stage, then the kernels' arithmetic (retto_amd/csrc/jpeg_recon.h)
 * run on the CPU; *on_device tells whether the device path would take the page (otherwise *rgb is the host decode).  GPU-free,
 * sessionless; *rgb is library-owned until rt_buffer_free. */
RT_API int rt_submit_encoded_batch(rt_session* s, const void* const* files, const size_t* lens, int n_pages, rt_ticket** out);
RT_API int rt_decode_batch(rt_session* s, const void* const* files, const size_t* lens, int n, int* hs, int* ws,
                           uint8_t* const* out, int mem, int* on_device);
RT_API int rt_debug_jpeg_reconstruct(const void* data, size_t len, uint8_t** rgb, int* h, int* w, int* on_device, char* err,
                                     size_t err_cap);
/* RecCharacter::new (retto-core/src/processor/rec_processor.rs:29-46) on the bytes of ppocr_keys_v1.txt, with
 * Rust's semantics: strict String::from_utf8 (RT_ERR_UTF8 on overlong forms, surrogates, > U+10FFFF), str::lines,
 * str::trim over the Unicode White_Space set (a U+3000-only line becomes ""), "blank" inserted at 0 and " "
 * appended.  *out = the entries joined by '\n' (library-owned until rt_buffer_free), *n_entries their count.
 * Host-only; rt_create runs the same code on rt_config.dict. */
RT_API int rt_parse_dictionary(const void* data, size_t len, char** out, size_t* out_len, int* n_entries, char* err, size_t err_cap);
/* The JSON text of one f32 as serde_json (ryu) writes it -- shortest round-trip digits, "1.0" / "0.9" /
 * "1.234e-7", null for non-finite -- which rt_results_json uses for every number.  Returns the length. */
RT_API int rt_format_f32(float v, char* buf, size_t cap);
/* The tensor list (RTWB names and shapes, forward order, -1 = read from the file) the importer
 * fills for model `which`, one "name d0 d1 ..." line per tensor; returns the length needed. */
RT_API size_t rt_model_manifest(int which, char* buf, size_t cap);

/* ---- multi-GPU: the one collective of the design ------------------------------------------------------------
 * Pages shard over the GPUs of a node, one process (one rt_session) per GPU, with no data-path collective; the model blobs are
 * broadcast ONCE from `root` over RCCL (xGMI).  The reference has no counterpart (retto-cli/src/main.rs:80-86 is a serial loop
 * in one process).  rt_rccl_unique_id: rank `root` creates the 128-byte RCCL id and hands it to the other ranks out of band
 * (file / pipe / environment / MPI).  rt_broadcast_blobs: every rank calls it with the same id, world and root; on `root`
 * data[i] / lens[i] are the blobs to send (caller-owned), on the other ranks they are OUTPUTS: data[i] is library-allocated
 * (release with rt_buffer_free) and lens[i] its size.  The blobs then go into rt_config.{det,cls,rec,dict}.  librccl.so is
 * loaded on first use only.  err (optional) receives the failure message. */
RT_API int rt_rccl_unique_id(void* id, size_t cap, char* err, size_t err_cap);
RT_API int rt_broadcast_blobs(const void* id, int rank, int world, int device_id, int root, int n_blobs, void** data, size_t* lens,
                              char* err, size_t err_cap);

/* ---- diagnostics for tools/ (kernel A/B switches and the GEMM micro-benchmark; no reference
 * counterpart, not needed by a drop-in host) ------------------------------------------------
 * rt_debug_set_variants: gemm_variant 0 = production dispatch, 8 / 10 / 15 / 20 force the
 * 128x128 / 128x240 / 256x240 wide tiles / the streaming kernel; dw_variant has no effect;
 * flags bits: 0-5 no effect (their depthwise / thin-block variants were removed), 6 CTC head on
 * the 128x128 wide tile, 7 thin
 * LCNetV3 blocks back on k_lc_thin / the unfused pair (instead of k_lc_lds), 8 the wide fp32 GEMM
 * back on the register-staged tile (instead of k_gemm32p), 9 5x5 depthwise back on
 * k_dwconv_rows (instead of the column sweep), 10 the angle classifier's blocks as the unfused launch
 * series (instead of k_cls_block), 11 the RSEFPN output convs and the DB head conv as the round-3 launch
 * series over materialised upsampled tensors (instead of the upsampling-aware k_fpn_phase / k_fpn_class /
 * k_fpn_compose).
 * Process-wide; every setting but bits 10 and 11 computes bit-identical results (tests/test_gpu_parity.py
 * checks bits 7-9 on whole networks; bit 10 changes the order of the squeeze-excite pooling sums:
 * equal within 1e-6 on the class probabilities; bit 11 changes the summation order of the pre-summed phase
 * weights: equal within 2e-5 on the DB probability map). */
RT_API void rt_debug_set_variants(int gemm_variant, int dw_variant, int flags);
/* one launch of the fp16 implicit-GEMM conv kernel on host tensors: x [n, cin, h, w], wt [cout, cin, kh, kw], bias [cout] or
 * NULL, "same" padding k/2, stride (sh, sw), act = 0 none / 1 relu / 2 hardswish / 3 swish / 4 sigmoid -> out [n, cout, ho, wo] */
RT_API int rt_debug_conv16(rt_session* s, const float* x, int n, int cin, int h, int w, const float* wt, int cout, int kh, int kw,
                           int sh, int sw, const float* bias, int act, float* out);
/* times nn::gemm (M x K x N, random data) over `iters` launches on the session's stream and
 * returns the average ms and the max |diff| against variant 0 */
RT_API int rt_bench_gemm(rt_session* s, long long M, int K, int N, int variant, int iters, float* ms_out, float* maxdiff_out);
/* Error of one nn::gemm variant against an fp64 product on operands with full 24-bit significands (bias 0): out4 = {max |err|,
 * rms err, max |ref|, rms ref} over `rows` rows from the start, the middle and the end of the M rows.  variant 1 = narrow fp32-MFMA
 * kernel, 30 = k_gemm32p (fp32 MFMA), 40 = split-bf16 (three bf16 planes per operand, six bf16 MFMAs per product, fp32 accumulate). */
RT_API int rt_bench_gemm_err(rt_session* s, long long M, int K, int N, int variant, int rows, int act, unsigned seed, double* out4);
/* One nn::gemm launch on host arrays, for the numerics tests: out[:, coff ..] = epi(A x W + bias) (+ residual), as the networks
 * call it.  A [M][lda] (channels K .. lda zero), W [K][N] (packed as pack_linear packs a linear layer), bias [N] or NULL, act
 * (as rt_debug_conv16), LAB (has_lab, lab_a, lab_c), residual [M][ld_res] or NULL.  Squeeze-excite: se_scale [n_img][ld_scale]
 * (NULL: none) over img_rows[n_img] consecutive images of M rows in all; se_rows = the row-block table's form (0 = what the
 * networks ask for, 128 or 256).  variant: 0 = production rule, else as rt_bench_gemm.  ctc = -1: the plain GEMM; 0 / 1 / 2: the
 * CTC head with that argmax form (idx_out / prob_out [M]: argmax and its softmax probability per row).  out [(M + 64) * ldc] is
 * filled with RT_DEBUG_CANARY before the launch and returned whole.  plan_out[5] = {GemmKernel value (gemm_plan.h), nt, kg, se,
 * bf} of the plan that ran. */
#define RT_DEBUG_CANARY 0x7FA5C3E1u
RT_API int rt_debug_gemm(rt_session* s, const float* A, long long M, int K, int lda, const float* W, int N, const float* bias,
                         int act, int has_lab, float lab_a, float lab_c, const float* residual, int ld_res, const float* se_scale,
                         int ld_scale, const long long* img_rows, int n_img, int se_rows, int ldc, int coff, int variant, int ctc,
                         float* out, int* idx_out, float* prob_out, int* plan_out);
/* One depthwise conv layer (K = 3 or 5, stride (sh, sw) in {1, 2}, "same" padding) on host arrays, for the numerics tests: n_img
 * images of heights[i] x widths[i] pixels, consecutive in x [sum h w][Cp] (channels C .. Cp: anything, the output's are +0); w [K * K][Cp] (tap dy * K + dx),
 * bias [Cp]; act / LAB as rt_debug_gemm.  form: 0 = the row-strip kernel, 1 = the column-sweep kernel where the layer has an
 * instance (info_out[3] tells).  out [(sum ho wo + 64) * Cp], filled with RT_DEBUG_CANARY before the launch and returned whole.
 * pooled != 0: the kernel also leaves the squeeze-excite partial sums, returned as they lie in memory in partial_out
 * [n_img][chunks][Cp] (canary where nothing was written; partial_cap = floats available) and, in mean_out [n_img][Cp], as the
 * channel means the squeeze-excite FC reads from them.  info_out[4] = {chunks, strip rows, strips per block, sweep ran}; the launch
 * follows the plan rt_debug_dw_plan reports for the same arguments. */
RT_API int rt_debug_dwconv(rt_session* s, const float* x, const int* heights, const int* widths, int n_img, int C, int Cp, int K,
                           int sh, int sw, const float* w, const float* bias, int act, int has_lab, float lab_a, float lab_c,
                           int pooled, int form, float* out, float* partial_out, long long partial_cap, float* mean_out,
                           int* info_out);
/* One nn::attention launch (head dim 15) on host arrays: qkv [rows][3 * heads * 15] (q | k | v, as the neck's qkv GEMM writes
 * it), lines of tokens[i] consecutive rows (sum = rows) -> out [rows][heads * 15], with the geometry SvtrCore::mixer passes. */
RT_API int rt_debug_attention(rt_session* s, const float* qkv, long long rows, const int* tokens, int n_lines, int heads,
                              float* out);
/* One fused thin LCNetV3 block (3x3 depthwise, stride (sh, sw), "same" padding -> 1x1 conv + hardswish) through the networks' run_lc on
 * host arrays, for the numerics tests: n_img images of heights[i] x widths[i] pixels, consecutive in x [sum h w][Cp] with Cp =
 * cin rounded up to 4 (32 from 128 channels on; channels cin .. Cp zero), laid out as the networks' levels are.  dw_w [cin][3][3]
 * (torch depthwise layout) and dw_bias [cin], pw_w [cout][cin] and pw_bias [cout], packed by the networks' own packers; dw_act and
 * the two LABs (has, a, c) as rt_debug_gemm.  form (the thin blocks' A/B switch): 0 = k_lc_thin, or the depthwise + GEMM pair where
 * it has no instance, 1 = k_lc_wave, 3 = k_lc_lds (production).  out [(sum ho wo + 64) * ldy], ho = ceil(h / sh), wo = ceil(w / sw),
 * ldy = cout's channel pitch, filled with RT_DEBUG_CANARY before the launch and returned whole.  info_out[0] = the route that ran:
 * 0 the unfused pair, 1 k_lc_thin, 2 k_lc_wave, 3 k_lc_lds. */
RT_API int rt_debug_lc_block(rt_session* s, const float* x, const int* heights, const int* widths, int n_img, int cin, int cout,
                             int sh, int sw, const float* dw_w, const float* dw_bias, const float* pw_w, const float* pw_bias,
                             int dw_act, int dw_has_lab, float dw_a, float dw_c, int pw_has_lab, float pw_a, float pw_c, int form,
                             float* out, int* info_out);
/* The plan rt_debug_dwconv launches by (nn::dw_plan under the depthwise form `form`: 0 = row strips only, 1 = the column sweep where
 * the layer has an instance) for a K x K depthwise conv, stride (sh, sw), channel pitch Cp, onto images of at most maxHo x maxWo
 * OUTPUT pixels; pooled != 0: with the squeeze-excite partial sums.  Host only: it takes no session and touches no device.
 * plan_out[8] = {kernel (0 invalid, 1 k_dwconv_rows on 32-channel slabs, 2 on 64-channel slabs, 3 k_dwconv_sweep), instance (sweep:
 * 1 - 6; rows: (((lanes * 8 + K) * 8 + R) * 4 + sh) * 4 + sw), strip rows R, lanes per pixel, strips per block, partial sums per image
 * (chunks), grid x, grid z}; the grid's y is the image count. */
RT_API int rt_debug_dw_plan(int K, int sh, int sw, int Cp, int maxHo, int maxWo, int pooled, int form, int* plan_out);
/* One wide LCNetV3 block (K x K depthwise, K = 3 or 5, stride (sh, sw), "same" padding [-> squeeze-excite] -> 1x1 conv + hardswish)
 * through the networks' run_lc on host arrays, for the numerics tests: the sibling of rt_debug_lc_block for the blocks that entry
 * cannot express.  x [sum h w][Cp], Cp = cin's channel pitch; channels cin .. Cp may hold anything.  dw_w [cin][K][K], dw_bias
 * [cin], pw_w [cout][cin], pw_bias [cout], the two LABs as rt_debug_lc_block.  Squeeze-excite: fc1_w [cin / 4][cin], fc1_b [cin / 4],
 * fc2_w [cin][cin / 4], fc2_b [cin] (hard-sigmoid slope 1/6), all four or all NULL.  dw_form: the depthwise form as rt_debug_dwconv's;
 * the GEMM runs under variant 0 (the production rule).  Three buffers come back whole, each filled with RT_DEBUG_CANARY before the
 * launch and 64 rows longer than its data: out [(sum ho wo + 64) * ldy] (ldy = cout's channel pitch), y1_out [(sum ho wo + 64) * Cp]
 * = the depthwise buffer handed to run_lc (unscaled where the squeeze-excite is folded into the GEMM, scaled in place otherwise),
 * scale_out [(n_img + 64) * Cp] = the per-image scales (NULL and 0 without squeeze-excite).  info_out[16] = {route (as
 * rt_debug_lc_block), then of the unfused route: depthwise kernel, instance, R, lanes, strips per block, chunks, grid x, grid z (as
 * rt_debug_dw_plan), rows of the squeeze-excite table folded into the GEMM (0: not folded), GemmKernel value of the pointwise GEMM's
 * plan, that plan's se flag, scales: 0 none, 1 folded, 2 applied in place; the rest 0}.  The session is looked at last. */
RT_API int rt_debug_lc_wide(rt_session* s, const float* x, const int* heights, const int* widths, int n_img, int K, int cin, int cout,
                            int sh, int sw, const float* dw_w, const float* dw_bias, const float* pw_w, const float* pw_bias, int dw_act,
                            int dw_has_lab, float dw_a, float dw_c, int pw_has_lab, float pw_a, float pw_c, const float* fc1_w,
                            const float* fc1_b, const float* fc2_w, const float* fc2_b, int dw_form, float* out, long long out_len,
                            float* y1_out, long long y1_len, float* scale_out, long long scale_len, int* info_out);
/* One 1x3 conv over lines of tokens (the SVTR neck's) on host arrays: x [rows][ldx] (channels 0 .. cin read), lines of
 * tokens_per_line[i] consecutive rows (sum = rows), w [cout][cin][1][3], bias [cout] or NULL, zero padding at both ends of every
 * line, act as rt_debug_gemm.  form 0 = nn::conv_sp on one 1 x T image per line, 1 = nn::conv13_flat over the flat token list with
 * the line-boundary flags the recognition net builds.  out [(rows + 64) * ldy], ldy = cout's channel pitch, filled with
 * RT_DEBUG_CANARY before the launch and returned whole.  info_out[2] = {column tiles per workgroup conv13_flat chose (0 for form
 * 0), the CU count it chose them for}. */
RT_API int rt_debug_conv13(rt_session* s, const float* x, long long rows, int ldx, const int* tokens_per_line, int n_lines, int cin,
                           const float* w, int cout, const float* bias, int act, int form, float* out, int* info_out);
/* One nn::add_layernorm launch on host arrays: out = LayerNorm(x + r) over the C channels of each row (r NULL: of x), x, r
 * [rows][C], g, beta [C].  out [(rows + 64) * C], filled with RT_DEBUG_CANARY before the launch and returned whole. */
RT_API int rt_debug_layernorm(rt_session* s, const float* x, const float* r, long long rows, int C, const float* g,
                              const float* beta, float eps, float* out);
/* One launch of a glue kernel of the fp16 family on host arrays, for the numerics tests.  n_img source images of src_h[i] x
 * src_w[i] pixels and n_img destination images of dst_h[i] x dst_w[i] pixels, each list consecutive in its buffer as the
 * networks' levels are.  All host arrays are float32 and hold whole buffers, row by row; the entry converts to and from fp16 (and to
 * bytes for op 11) where the kernel's operand is one.  ip[0] = channels processed (C or Cp), ip[1] = source pitch, ip[2] = source
 * channel offset, ip[3] = destination pitch, ip[4] = destination channel offset; ip[5 .. 11] and fp[0 .. 6] per op:
 *    0 dwconv16          x [ps][ip1] -> out; ip5.. = K, sh, sw, act, has_lab; fp = lab_a, lab_c; tab = w [K * K][C] then bias [C]
 *    1 global_mean16     x [ps][ip1] -> fp32 out [n_img][C] (ip3 = C)
 *    2 gate16            fp32 x [n_img][ip1] -> fp32 out [n_img][ip3]; ip0 = C, ip3 = Cp, ip5 = residual; fp0 = slope (< 0: sigmoid)
 *    3 scale_channels16  ip5 = the residual's pitch (0: none; x2 [ps][ip5]), ip6 = its channel offset, ip7 = in place (the output
 *                        buffer starts as x and is also read); tab = scale [n_img][C]
 *    4 upsample_add16    x = b [ps][C] (low resolution), x2 = a [pd][C]; ip5 = in place on a, ip6 = tab holds scale_a [n_img][C]
 *    5 upsample_into16   ip5 = shift, ip6 = the scale table's pitch (0: no scale); tab = scale [n_img][ip6]
 *    6 maxpool16         ip5.. = kh, kw, sh, sw, ph, pw
 *    7 avgpool16         ip5.. = kh, kw (window = stride; dst * k <= src)
 *    8 pixel_shuffle16   x [ps][ip1] holding 4 * C channels from ip2 on; dst <= 2 * src
 *    9 deconv_to_map16   x = f [ps][ip1], tab = w [C][4], fp0 = b -> fp32 out [pd] (ip3 = 1); dst = 2 * src
 *   10 map_window16      fp32 x = map [ps] (ip0 = 16, ip1 = 1), src = the map's images, dst = the feature images; 16 channels at ip4
 *   11 u8_to_h8          x [ps][3] byte values (ip0 = 8, ip1 = 3, ip3 = 8); fp0 = scale, fp1..3 = mean, fp4..6 = std; page i is
 *                        written from the first pixel of destination image i (dst pixels >= src pixels)
 *   12 f32x4_to_h8       fp32 x [ps][4] -> out [ps][8] (ip0 = 8, ip1 = 4, ip3 = 8)
 *   13 h_to_f32, 14 f32_to_h   x [ps][ip1] -> out [ps][ip3] at channel offset ip4, C = ip0 channels
 * ps / pd = the pixels of all source / destination images.  out [(rows + 64) * pitch] (rows = pd, or ps / n_img as above) is
 * filled with RT_DEBUG_CANARY before the launch and returned whole; for fp16 outputs every 32-bit canary word is two halves,
 * returned converted like the rest.  x_len, x2_len, tab_len, out_len = the arrays' lengths in floats: everything the kernel
 * can address is checked against them before any device work. */
RT_API int rt_debug_glue16(rt_session* s, int op, const int* ip, const float* fp, const int* src_h, const int* src_w,
                           const int* dst_h, const int* dst_w, int n_img, const float* x, long long x_len, const float* x2,
                           long long x2_len, const float* tab, long long tab_len, float* out, long long out_len);
/* One launch of a kernel of the fp32 detector's neck or head (nn_fpn.hip and the FPN glue of nn_kernels.hip) on host arrays, through
 * the launcher DetNet::run calls, for the numerics tests.  n_img images of fine_h[i] x fine_w[i] pixels are the op's finest
 * level and coarse_h / coarse_w the next coarser one where the op has one (always passed; ignored otherwise); levels below that
 * are derived by halving.  A coarse level that is not exactly half of its fine level is rejected: DetNet::run never passes one.
 * in[10] / in_len[10] are the operand arrays (float32, whole buffers, lengths in floats; NULL / 0 where the op or its flags do not
 * use a slot), out[3] / out_len[3] the outputs: each is filled with RT_DEBUG_CANARY before the launch, has 64 spare rows past its
 * last one and is returned whole.  Weights arrive in torch layout and go through the packers of the networks (pack_conv,
 * fpn_fine_weights, fpn_phase_weights, fpn_class_weights, fpn_lateral_weights, fpn_tap_weights); w = a 3x3 conv [24][96][3][3],
 * lat = a bias-free lateral 1x1 conv [96][cin].  pf / pc = pixels of all fine / coarse images, cf = cin rounded up to 4.
 *   op 0 phase         ip = {cin, cc, flags}: flags 1 bias, 2 pool, 4 relu, 8 G, 16 fine scale, 32 coarse scale, 64 compose first.
 *                      in: 0 fine [pf][cf], 1 coarse [pc][cc], 2 w, 3 bias [24], 4 Wf [n_img][9][24][cf] (cin < 24 without
 *                      compose), 5 lat, 6 lat scale [n_img][96] (compose: nn::fpn_compose runs first in the same call and its
 *                      output is the launch's Wf), 7 fine scale [n_img][24], 8 coarse scale [n_img][24], 9 G [9][pc / 4][24].
 *                      cin is 12, 18 or 24, nothing else.  cin = 24 is the head conv (cc = 24: fine = channels 72 .. 95 of w, coarse = 48 .. 71; scales and G only
 *                      here), cin < 24 an inp conv (cc = 96: coarse = all of w).  out: 0 y [(pf + 64) * 24], 1 the per-tile
 *                      pool sums [(n_img * tiles + 64) * 24] with tiles = those of the largest height x the largest width,
 *                      2 the composed weights [(n_img * 216 + 64) * cf].  info_out[0] = the k_fpn_phase instance as
 *                      CF4 * 100 + NS * 10 + HASG.
 *   op 1 class         ip = {c0, flags}: c0 = first of the 24 input channels of w, flags 1 bias, 2 scale, 4 lower.  in: 0 z [pf][24],
 *                      1 w, 2 bias, 3 scale [n_img][24], 4 lower [9][pc][24].  out: 0 V [(9 * pf + 64) * 24].
 *   op 2 compose       ip = {cin}, 12 or 18.  in: 0 lat, 1 scale [n_img][96], 2 w.  out: 0 [(n_img * 216 + 64) * cf].
 *   op 3 tail          nn::db_head_tail.  in: 0 x [pf][24], 1 deconv1 w [24][24][2][2], 2 its bias [24], 3 deconv2 w [24][1][2][2],
 *                      4 its bias [1].  out: 0 the map at four times the fine sides [16 * pf + 1024].
 *   op 4 lateral_add   ip = {cin, has b}.  in: 0 x [pf][cf], 1 lat, 2 scale [n_img][96], 3 b [pc][96].  out: 0 [(pf + 64) * 96].
 *   op 5 upsample_add  ip = {in place, has scale}.  in: 0 a [pf][96], 1 b [pc][96], 2 scale [n_img][96].  out: 0 [(pf + 64) * 96]
 *                      (in place: the buffer holds a before the launch and is both operand and output).
 *   op 6 se_projected  ip = {cin, Cr, residual}, fp = {slope}.  in: 0 x [pf][cf], 1 lat, 2 fc1 w [Cr][96], 3 fc1 b, 4 fc2 w [96][Cr],
 *                      5 fc2 b.  out: 0 the scales [(n_img + 64) * 96].
 *   op 7 se_tiles      ip = {Cr, residual}, fp = {slope}.  in: 0 pool sums [n_img][tiles][24] as op 0 leaves them, 1 .. 4 the FCs for
 *                      24 channels.  out: 0 the scales [(n_img + 64) * 24].
 *   op 8 head_fused    nn::conv3_fpn_fused.  ip = {flags}: 1 / 2 / 4 / 8 scale of p5 / p4 / p3 / p2, 16 bias, 32 relu.  in: 0 .. 3
 *                      p5, p4, p3, p2 [pixels of the level][24] (fine = p2's level, sides multiples of 8), 4 w, 5 bias, 6 .. 9 the
 *                      scales [n_img][24].  out: 0 [(pf + 64) * 24].
 *   op 9 conv3         nn::conv_sp(3, 3) at 96 -> 24.  ip = {flags}: 1 bias, 2 relu.  in: 0 x [pf][96], 1 w, 2 bias.  out: 0
 *                      [(pf + 64) * 24].  info_out[0] = NG of the k_conv3_few<NG> instance that ran (0: k_conv_sp).
 * Everything the kernel can address is checked against the lengths before any device work, and like the two fp16 entries this
 * one looks at its session last. */
RT_API int rt_debug_fpn(rt_session* s, int op, const int* ip, const float* fp, const int* fine_h, const int* fine_w,
                        const int* coarse_h, const int* coarse_w, int n_img, const float* const* in, const long long* in_len,
                        float* const* out, const long long* out_len, int* info_out);
/* One nh::conv16 launch as the fp16 networks issue it, on host arrays, for the numerics tests.  n_img images of heights[i] x
 * widths[i] pixels, consecutive in x as a level is; the output images follow the networks' rule (ceil(side / stride); the input
 * geometry for the 2x2 phase convs).  ip[20] = cin, ldx, xoff (the input is channels [xoff, xoff + cin) of rows of pitch ldx),
 * cout, ldy, coff (the output goes to channels [coff, coff + pitch8(cout)) of rows of pitch ldy), kh, kw, sh, sw, pt, pl (-1 = k / 2),
 * flat (1: one image of 1 x total pixels, as the 1x1 layers are launched), act, has_lab, ld_res, res_off (the residual is
 * res [pixels][ld_res] from channel res_off on; res may be NULL), in_place (the output buffer starts as x and is the input
 * too; ldx == ldy), dot_py, dot_px.  fp[3] = lab_a, lab_c, dot_b.  wt [cout][cin][kh][kw], bias [cout] or NULL.  All host arrays
 * are float32; fp16 operands are converted.  out [(pixels_out + 64) * ldy] is filled with RT_DEBUG_CANARY (two halves a word)
 * before the launch and returned whole.  With dot_w [cout] (the PFHeadLocal phase convs: 2x2, pads 0 / 1, 33 .. 64 output
 * channels) nothing is stored: out [4 * pixels + 64] holds the fp32 map at twice the resolution on entry (its 64 spare floats
 * are overwritten with the canary), map[(2y + dot_py, 2x + dot_px)] = 0.5 * (map + sigmoid(dot_b + sum_n act(conv)[n] dot_w[n]))
 * is applied and the map is returned whole.  route_out receives the kernel that ran: 1 = k_conv16, 2 = k_conv16v2, 3 = k_gemm16p,
 * + 8 for an instance with the dot epilogue.  The two fp16 entries check their arguments before they look at the session, so
 * that each check answers with its own message (rt_last_error(NULL)) even where no session can be created. */
RT_API int rt_debug_conv16x(rt_session* s, const int* ip, const float* fp, const int* heights, const int* widths, int n_img,
                            const float* x, long long x_len, const float* wt, long long wt_len, const float* bias, const float* res,
                            long long res_len, const float* dot_w, float* out, long long out_len, int* route_out);
/* One MobileNetV3 inverted-residual block of the angle classifier (expand 1x1 -> depthwise k x k, stride (sh, 1) -> squeeze-excite
 * -> linear 1x1 [+ x]) on host arrays, through the function ClsNet::run calls per block, for the numerics tests.  n crops of one
 * H x W (the classifier never has ragged input), x [n H W][cin]; exp_w [mid][cin], exp_b [mid]; dw_w [mid][k][k] (torch depthwise
 * layout), dw_b [mid]; se != 0: fc1_w [mid / 4][mid], fc1_b [mid / 4], fc2_w [mid][mid / 4], fc2_b [mid] (hard-sigmoid slope 0.2,
 * offset 0.5); lin_w [cout][mid], lin_b [cout]; act = 1 relu / 2 hardswish on the expansion and the depthwise; the shortcut is
 * taken where sh == 1 and cin == cout.  cin, mid, cout are multiples of 4.  form: 0 = the launch series (GEMM, depthwise,
 * pooling + FCs, channel scaling, GEMM), 1 = the single k_cls_block launch where cls_block_supported() has an instance.
 * out [(n Ho W + 64) * cout], Ho = ceil(H / sh), filled with RT_DEBUG_CANARY before the launch and returned whole.
 * info_out[4] = {k_cls_block ran, its LDS slice has padded rows (0: XOR swizzle), row tiles per wave MAXU (9 or 5), LDS bytes};
 * all 0 where the series ran. */
RT_API int rt_debug_cls_block(rt_session* s, const float* x, int n, int H, int W, int cin, int mid, int cout, int k, int sh, int act,
                              int se, const float* exp_w, const float* exp_b, const float* dw_w, const float* dw_b, const float* fc1_w,
                              const float* fc1_b, const float* fc2_w, const float* fc2_b, const float* lin_w, const float* lin_b,
                              int form, float* out, int* info_out);
/* One stem launch (3x3 conv, stride 2, pad 1, 3 -> cout channels) on n_img images of heights[i] x widths[i] pixels, consecutive in
 * their buffer.  Exactly one of x4 / rgb is given: x4 = float32 NHWC-4 [pixels][4] (channel 3 ignored) with cout 8 (k_stem<8>, the
 * classifier's) or 16 (k_stem_mfma<0>, the rec net's); rgb = RGB8 pages [pixels][3] with cout 16 (k_stem_mfma<1>, the det net's:
 * tensor channel c = (byte[2 - c] * scale - mean3[c]) / std3[c], three separately rounded float32 operations).  w [cout][3][3][3],
 * bias [cout], act as rt_debug_gemm.  out [(sum ceil(h / 2) ceil(w / 2) + 64) * cout] (out_len floats), filled with
 * RT_DEBUG_CANARY before the launch and returned whole. */
RT_API int rt_debug_stem(rt_session* s, const float* x4, const unsigned char* rgb, const int* heights, const int* widths, int n_img,
                         int cout, const float* w, const float* bias, int act, float scale, const float* mean3, const float* std3,
                         float* out, long long out_len);
/* One launch of a glue kernel of the fp32 family on host arrays, for the numerics tests.  Ops 0 - 3 work on n_img images of
 * heights[i] x widths[i] pixels, consecutive in x [pixels][pitch]; ops 4 - 6 on n_img ROWS (heights / widths unused, may be NULL).
 *    0 se_scale          ip = {C, Cr, residual, apply}, fp = {slope}; x [pixels][Cp], Cp = C's channel pitch (C rounded up to 4; to
 *                        32 from 128 channels on); w[4] = fc1 w [Cr][C], fc1 b [Cr], fc2 w [C][Cr], fc2 b [C].  out = the scales
 *                        [(n_img + 64) * Cp] (channels C .. Cp: +0); apply: nn::scale_channels then multiplies x in place, out2 =
 *                        that buffer [(pixels + 64) * Cp]
 *    1 global_mean       ip = {Cp}; x [pixels][Cp] -> out [(n_img + 64) * Cp]
 *    2 maxpool_2x2       ip = {Cp}; images of at least 2 x 2 -> out [(sum floor(h / 2) floor(w / 2) + 64) * Cp]
 *    3 avgpool_3x2       ip = {Cp, ldy}; images of at least 3 x 2 -> channels 0 .. Cp of out [(sum floor(h / 3) floor(w / 2) + 64) * ldy]
 *    4 softmax_rows      ip = {C, ld}; x [rows][ld] -> out [(rows + 64) * C]
 *    5 argmax_prob_rows  ip = {C, ld} -> idx_out [rows + 64] (the first argmax), out [rows + 64] (its softmax probability)
 *    6 argmax_rows       ip = {C, ld} -> idx_out [rows + 64], out [rows + 64] (the maximum itself)
 * out, out2 and idx_out are filled with RT_DEBUG_CANARY before the launch and returned whole; x_len, out_len, out2_len = the
 * arrays' lengths in floats, checked before any device work.  The session is looked at last. */
RT_API int rt_debug_glue32(rt_session* s, int op, const int* ip, const float* fp, const int* heights, const int* widths, int n_img,
                           const float* x, long long x_len, const float* const* w, float* out, long long out_len, float* out2,
                           long long out2_len, int* idx_out);
/* times the fused thin LCNetV3 block (3x3 depthwise -> 1x1 conv; n images of h x w, random data).  form: 0 = k_lc_thin
 * (workgroup-staged; the unfused depthwise + GEMM pair where it has no instance), 1 = k_lc_wave (direct loads, stride 1 only),
 * 3 = k_lc_lds (production).  stride: 1, 2, or 21 = (2, 1).  Returns the average ms and the max |diff| against form 0. */
RT_API int rt_bench_lc(rt_session* s, int n, int h, int w, int cin, int cout, int stride, int form, int iters, float* ms_out, float* maxdiff_out);
/* The main lane's arenas (tools/bench_det_tiles.py): out3 = the largest pass so far, in bytes, of the call arena, of the scratch
 * arena (network activations, rewound per launch group) and of the DB post-processing workspace. */
RT_API int rt_debug_arena_high_water(rt_session* s, long long* out3);
/* iters device-to-device hipMemcpyAsync of `bytes` bytes on the session's stream, timed with events: *ms_out = the mean per copy. */
RT_API int rt_bench_memcpy_d2d(rt_session* s, size_t bytes, int iters, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* RETTO_HIP_H */

// Host scheduler: the MI355X counterpart of RettoSession::process_pipeline (retto-core/src/session.rs:75-106) over a batch of
// pages, plus the tensor-level worker entry points (worker.rs:69-73) and the stage functions.  A pipeline call travels as one
// value, PageCall; what runs it is a lane, rt_lane (stream, arenas, pinned staging, profile and the functions on that stream);
// the session, rt_session, is lane 0 plus what exists once: config, networks, dictionary, rec stores, the setters' defaults, the
// helper lanes with their threads, tickets and staging.  session.cpp: construction, the stage-level entries, the page pipeline;
// session_batch.cpp: lanes at work, tickets, staging, encoded pages; rec_tail.cpp: the rec CTC tail and the stores' create calls.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/retto_hip.h"
#include "image_decode.h"
#include "jpeg_recon.h"
#include "lane_split.h"
#include "nets.h"
#include "nets_f16.h"
#include "prepost.h"
#include "rec_line_opts.h"
#include "rec_tail_plan.h"
#include "runtime.h"

struct rt_results {
  struct Page {
    std::vector<float> boxes;        // n x 8, original-image coordinates
    std::vector<float> det_scores;
    std::vector<uint16_t> cls_labels;
    std::vector<float> cls_scores;
    std::vector<float> rec_scores;
    std::vector<std::vector<int32_t>> tokens;
    std::vector<std::string> text;
    // rt_config.rec_return_word_box: per line its words (quads in original-image coordinates) and their texts; empty when off
    std::vector<std::vector<rt::wb::Word>> words;
    std::vector<std::vector<std::string>> word_text;
    // rt_config.rec_return_candidates = cand_k > 0 (ctc_candidates.h): the page's kept tokens in line order, line k's from
    // cand_off[k] (one array per page, not per line: two allocations); their time steps and [cand_k] candidates each.  Empty when off
    int cand_k = 0;
    std::vector<uint32_t> cand_off;   // [lines + 1]
    std::vector<int32_t> cand_cols;
    std::vector<rt::cc::Cand> cands;
    // rec lexicons (ctc_lexicon.h): per line the lexicon it was scored against (0: none), its number of matches and
    // [rt::lx::MATCHES] match slots.  Empty when no line of the call carried a lexicon
    std::vector<int32_t> lex_id, lex_n;
    std::vector<rt::lx::Match> lex_matches;
    // lexicon snap (ctc_lexicon_align.h): per line 1 where its decode is its aligned best entry.  Empty when no lexicon of the
    // call's lines had snap on
    std::vector<uint8_t> lex_snapped;
    // rec patterns (ctc_pattern.h): per line its pattern (0: none) and result; empty when no line of the call carried one
    std::vector<int32_t> pat_id; std::vector<rt::pt::LineResult> pat_res;
    // rec keywords (ctc_keyword.h): per line its list (0: none), its number of hits and [rt::kw::HITS] hit slots, each with its
    // page quad; empty when no line of the call carried a list
    std::vector<int32_t> kw_id, kw_n;
    std::vector<rt::kw::Hit> kw_hits;
    // rec beams (ctc_beam.h; rt_set_rec_beam): beam_n = the call's hypotheses per line (0: off, everything below empty); per line
    // its count and [beam_n] record slots; hypothesis k of line l has its tokens and its text at [l * beam_n + k]
    int beam_n = 0;
    std::vector<int32_t> bm_count;
    std::vector<rt::bm::Beam> bm_recs;
    std::vector<std::vector<int32_t>> bm_tokens;
    std::vector<std::string> bm_text;
    // rec language model (ctc_lm.h; rt_set_rec_beam_lm): per record slot the hypothesis' lm and fused score; empty when fusion was off
    std::vector<rt::lm::BeamLm> bm_lm;
    // rec vocabulary (ctc_vocab.h; rt_set_rec_beam_vocab): per record slot the hypothesis' closed count and closing score; empty
    // when no vocabulary was attached
    std::vector<rt::vc::BeamVocab> bm_vocab;
    // rec windows (rec_windows.h; rt_set_rec_windows): per line the number of units it was read in, 1 for a whole line
    std::vector<int32_t> rec_units;
    // rec flip (rec_flip.h; rt_set_rec_flip): per line its outcome (0: read one way, 1: both ways and view 0 kept, 2: view 1
    // taken) and the two views' greedy scores [2 per line]; empty when no line of the call was read both ways
    std::vector<uint8_t> flip_outcome; std::vector<float> flip_scores;
    std::string json[3];
  };
  std::vector<Page> pages;
  double det_checksum = 0.0;
};

// A lane's host thread: created once per session (rt_session::ensure_workers), parked on a condition variable between jobs.
// Jobs run in submission order; a lane works through the parts of consecutive batches back to back, so the result assembly of
// batch i (host) and the det phase of batch i + 1 overlap with the other lanes' kernels.
struct LaneWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::function<void()>> q;
  bool stop = false;
  void start(int device);
  void push(std::function<void()> f);
  void shutdown();
  ~LaneWorker() { shutdown(); }
};

// What a pipeline call reads of the session's settings, as they were when the call was submitted: the default options of every
// line (rt_set_rec_charset / _lexicon / _pattern / _keywords, rec_line_opts.h), the det tiles (rt_set_det_tiles, det_tiles.h; 0 = off)
// the rec beam (rt_set_rec_beam, ctc_beam.h; beam_b = 0: off), the rec windows (rt_set_rec_windows, rec_windows.h; 0 = off) and
// the beam's language model (rt_set_rec_beam_lm, ctc_lm.h; lm = -1: off, and without effect while beam_b = 0) and its word list
// (rt_set_rec_beam_vocab, ctc_vocab.h; beam_vocab = -1: off, likewise), and the rec flip (rt_set_rec_flip, rec_flip.h; 0 = off).
// With 0 < flip_cls_below <= 1 the call syncs its lane once more, between the cls stage and the rec plan, to bring the
// classifier scores to the host
struct CallSettings {
  rt::RecLineOpts rec; int det_tile = 0, det_overlap = 0, beam_b = 0, beam_n = 0, rec_window = 0, rec_overlap = 0;
  int lm = -1; float lm_alpha = 0.0f, lm_beta = 0.0f;
  int beam_vocab = -1; float vocab_gamma = 0.0f;
  float flip_cls_below = 0.0f;
  bool fused() const { return beam_b > 0 && lm >= 0; }
  bool worded() const { return beam_b > 0 && beam_vocab >= 0; }
};

// One pipeline call over some pages: what rt_lane::run_pages runs, whoever asked for it (rt_run_batch, rt_submit_batch,
// rt_run_regions*, a lane's part of a ticket).  Non-owning: every array has n_pages entries and belongs to the caller or the ticket.
struct PageCall {
  int n_pages = 0, mem = RT_MEM_HOST;
  const uint8_t* const* rgb = nullptr;
  const int* hs = nullptr;
  const int* ws = nullptr;
  const float* const* det_map_override = nullptr;   // or null
  // rt_run_regions*: per page its quads (n_quads[i] x 8 floats, validated and clamped), their number and the regions' options,
  // resolved (no -1) and checked (rt::resolve_region_opts); n_quads null: the detector finds the boxes; opts null: every line set.rec
  const float* const* quads = nullptr;
  const int* n_quads = nullptr;
  const rt::RecLineOpts* const* region_opts = nullptr;
  CallSettings set;
  // run_stream (session.rs:133-143): stage results are handed to the callback as soon as the stage is complete -- Det after the
  // box round trip (before any crop is classified or read), Cls and Rec when the call ends.  cb_mu (or null) serialises the
  // callbacks of concurrent lanes; page_base = the global index of the call's first page
  rt_stage_callback cb = nullptr;
  void* user = nullptr;
  std::mutex* cb_mu = nullptr;
  int page_base = 0;
  bool on_lane_worker = false;   // the call runs on a lane's worker thread (a submitted batch): only the spin window reads it
  bool regions() const { return n_quads != nullptr; }
  // the sub-call over pages [f0, f1)
  PageCall part(int f0, int f1) const {
    PageCall c = *this;
    c.n_pages = f1 - f0; c.rgb += f0; c.hs += f0; c.ws += f0; c.page_base += f0;
    if (det_map_override) c.det_map_override += f0;
    if (quads) c.quads += f0;
    if (n_quads) c.n_quads += f0;
    if (region_opts) c.region_opts += f0;
    return c;
  }
};

// One submitted batch (rt_submit_batch): the argument arrays are copied (the PAGES must stay valid until rt_wait_batch), the
// pages are split over the lanes exactly as rt_run_batch splits them, each lane leaves its part here.
struct rt_ticket {
  int nl = 0;
  // what must outlive the submitting call, and the call over it as the lanes run it: on a lane's thread, with mem = pages on the
  // device once they are staged (the regions' arrays stay the caller's: rt_run_regions* waits)
  std::vector<const uint8_t*> rgb;
  std::vector<int> hs, ws;
  std::vector<const float*> maps;   // empty: no override
  PageCall call;
  std::vector<int> first;
  std::vector<rt_results*> parts;
  std::vector<std::exception_ptr> errs;
  std::mutex cb_mu;                 // callbacks of concurrent lanes are serialised
  std::mutex mu;
  std::condition_variable cv;
  int remaining = 0;
  // host pages staged by rt_submit_batch itself (session_batch.cpp "page staging"): rgb[] then holds device addresses inside the
  // session's staging slot `stage_slot`, and the lanes wait for `ev_up` on their streams instead of copying
  int stage_slot = -1;
  std::vector<size_t> stage_off;    // per page: offset inside the slot, (size_t)-1 = not staged (empty page)
  std::vector<hipEvent_t> ev_up;    // per lane part; owned by the staging slot
  // rt_submit_encoded_batch: the ticket owns the host-decoded pages (coefficients or pixels); stage_part uploads lane part l and
  // reconstructs its JPEG pages with jpeg_kernels.hip into the slot before recording ev_up[l]
  std::vector<rt::EncodedPage> enc;
  struct EncPart {
    std::vector<rt::jpeg::DevComp> comps;
    std::vector<rt::jpeg::DevPage> pages;
    size_t comps_off = 0, pages_off = 0;   // the two tables inside the slot
    int blocks = 0;
    int64_t pixels = 0;
  };
  std::vector<EncPart> enc_parts;   // per lane part
};

// The session's rec charsets (ctc_charset.h), shared with the helper lanes.  Set k (1-based, rt_charset_create's id) has its
// sorted class ids in ids[k - 1] and its mask at d_masks + (k - 1) * words.  Only changed while no ticket is in flight and every
// lane's stream is drained (rt_charset_create is a guarded call), with a blocking copy.
struct rt_charsets {
  int words = 0;
  std::vector<std::vector<int32_t>> ids;
  uint32_t* d_masks = nullptr;   // [rt::cs::MAX_SETS][words], allocated by the first rt_charset_create
  ~rt_charsets() { if (d_masks) (void)hipFree(d_masks); }
};

// Lists of entries compiled by rt::compile_lexicon: what the rec lexicons and the rec keyword lists both are.  List k (1-based,
// the id add() returns) is host[k - 1] on the host (stable addresses: the rt_*_entry / _entry_text calls hand them out) and list
// k - 1 of `tb`, whose four tables sit on the device as `d`.
struct rt_entry_store {
  struct Host { std::vector<int32_t> ids, lens, off; std::vector<std::string> text; };
  std::vector<std::unique_ptr<Host>> host;
  rt::lx::Tables tb;
  rt::lx::DevTables d{};
  // what the rt_*_entries / _entry / _entry_text calls answer: list id (null: unknown), its number of entries, entry e's length
  // and ids, its text (0 / null: no such list or entry)
  const Host* list(int id) const { return id < 1 || id > (int)host.size() ? nullptr : host[(size_t)id - 1].get(); }
  int entries(int id) const { return list(id) ? (int)list(id)->lens.size() : 0; }
  int entry(int id, int e, const int32_t** ids_out) const {
    if (e < 0 || e >= entries(id)) return 0;
    if (ids_out) *ids_out = list(id)->ids.data() + list(id)->off[(size_t)e];
    return list(id)->lens[(size_t)e];
  }
  const char* entry_text(int id, int e) const { return e < 0 || e >= entries(id) ? nullptr : list(id)->text[(size_t)e].c_str(); }
  // Compiles the entries (rt::compile_lexicon over `dict`), builds their host record, rebuilds the tables whole and puts them
  // on the current device with set(); returns the new list's id.  Whatever throws leaves the store as it was.
  int add(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n);
  // `fresh` in four device allocations of its own in place of the tables there are, then tb = fresh: a throwing copy leaves the
  // old ones.  (The rt_debug_ctc_* hooks put their tables on the device with it too.)
  void set(rt::lx::Tables fresh);
  ~rt_entry_store();   // (never copied: `host` cannot be)
};

// The session's rec lexicons (ctc_lexicon.h), shared with the helper lanes: the store and the snap thresholds.  Only changed
// while no ticket is in flight and every lane's stream is drained (rt_lexicon_create is a guarded call), with blocking copies.
struct rt_lexicons : rt_entry_store {
  // lexicon snap (ctc_lexicon_align.h, rt_lexicon_set_snap): min_posterior per lexicon, 0 = never snap; d_snap [MAX_LEXICONS]
  // is allocated by the first rt_lexicon_set_snap and changed under the same guard, with a blocking copy
  float snap[rt::lx::MAX_LEXICONS] = {};
  float* d_snap = nullptr;
  ~rt_lexicons() { if (d_snap) (void)hipFree(d_snap); }
};

// The session's rec patterns (ctc_pattern.h), shared with the helper lanes.  Pattern k (1-based, rt_pattern_create's id) is
// host[k - 1] (stable addresses: rt_pattern_text hands the text out) and pattern k - 1 of `tb`, whose tables sit on the device as
// `d`.  Only changed while no ticket is in flight and every lane's stream is drained (rt_pattern_create is a guarded call): the
// tables are rebuilt and copied whole, with blocking copies.
struct rt_patterns {
  struct Host { std::string text; int S, P, min_steps; };
  std::vector<std::unique_ptr<Host>> host;
  rt::pt::Tables tb;
  rt::pt::DevTables d{};
  void free_device() {
    const void* p[] = {d.pats, d.pair_c, d.pair_pb, d.pair_pe, d.seg, d.preds};
    for (const void* q : p) if (q) (void)hipFree(const_cast<void*>(q));
    d = rt::pt::DevTables{};
  }
  ~rt_patterns() { free_device(); }
};

// The session's rec keyword lists (ctc_keyword.h), shared with the helper lanes: the store and the lists' min_score, on the
// device as d_min [lists].  Only changed while no ticket is in flight and every lane's stream is drained (rt_keywords_create is
// a guarded call), with blocking copies.
struct rt_keywords : rt_entry_store {
  std::vector<float> min_score;
  const float* d_min = nullptr;
  ~rt_keywords() { if (d_min) (void)hipFree(const_cast<float*>(d_min)); }
};

// The session's rec language models (ctc_lm.h), shared with the helper lanes.  Model k (0-based, rt_lm_create's handle) is
// host[k], whose three tables sit on the device as dev[k], uploaded once at creation and kept until the session goes.  Only
// changed while no ticket is in flight (rt_lm_create is a guarded call), with blocking copies.
struct rt_lms {
  std::vector<std::unique_ptr<rt::lm::Model>> host;
  std::vector<rt::lm::View> dev;
  // the model's tables onto the current device; returns its handle.  Whatever throws leaves the store as it was.
  int add(rt::lm::Model m);
  ~rt_lms();
};

// The session's rec vocabularies (ctc_vocab.h), shared with the helper lanes.  Vocabulary k (0-based, rt_vocab_create's handle) is
// host[k], whose four tables sit on the device as dev[k], uploaded once at creation and kept until the session goes.  Only
// changed while no ticket is in flight (rt_vocab_create is a guarded call), with blocking copies.
struct rt_vocabs {
  std::vector<std::unique_ptr<rt::vc::Vocab>> host;
  std::vector<rt::vc::View> dev;
  // the vocabulary's tables onto the current device; returns its handle.  Whatever throws leaves the store as it was.
  int add(rt::vc::Vocab m);
  ~rt_vocabs();
};

// internal to the library (never accepted from a caller): pages already in HBM, det map overrides still host pointers
#define RT_MEM_STAGED_MAPS_HOST 3

// One lane of a session: a stream with the arenas, pinned staging and profile of the calls that run on it, and the functions that
// run on that stream.  Lane 0 is the session itself (rt_session derives from rt_lane: the entry points and the debug hooks use
// s->st, s->arena ...); the others are the session's helper lanes, which rt_run_batch / rt_submit_batch give parts of a batch on
// concurrent host threads.  What every lane reads and none owns -- config, networks, dictionary, rec stores -- is the session's.
struct rt_session;
struct rt_lane {
  const rt_session* sh = nullptr;  // the session's shared state
  hipStream_t st = nullptr;        // the stream the lane's current call runs on: st_full, or st_part inside a multi-lane batch
  hipStream_t st_full = nullptr;   // whole device
  hipStream_t st_part = nullptr;   // this lane's CU partition (runtime.h "CU partitions"); nullptr: not partitioned
  int part_cus = 0;
  hipEvent_t ev_block = nullptr;   // blocking-sync event behind sync(): the lane's host thread sleeps instead of spinning
  int* d_flags = nullptr;          // [0] thumbnail/resize error flag
  rt::Arena arena;      // lives for one API call: pages, maps, crops, descriptors, outputs
  rt::Arena scratch;    // network activations; rewound per launch group
  rt::Arena dbws;       // DB post-processing workspace (stream-ordered reuse across pages)
  rt::Pinned pinned;
  rt::Profiler prof;
  int spin_us = 5000;              // sync(): how long to poll before sleeping; run_pages chooses it per call
  bool failed = false;             // the lane's previous call threw: its arena statistics are discarded at the next begin_call
  std::chrono::steady_clock::time_point last_exit = std::chrono::steady_clock::now();  // RT_TRACE only
  // the lane's stream, flag word and blocking event on the session's device (which is current), and their release
  void open(const rt_session* session);
  void close();

  rt::RunCtx ctx(rt::Arena* a) { return rt::RunCtx{st, a, &pinned, &prof}; }
  void begin_call();
  void sync();
  void check_flags();

  // L1
  void det_forward(const float* nchw, int n, int h, int w, float* out);
  void cls_forward(const float* nchw, int n, int h, int w, float* out);
  void rec_forward(const float* nchw, int n, int h, int w, float* out, int* t_out);
  void rec_forward_ragged(const float* nchw, int n, const int* widths, float* out, int* t_out);
  // stages
  void resize_both(const uint8_t* rgb, int h, int w, uint8_t* out, int oh, int ow);
  void det_preprocess(const uint8_t* rgb, int h, int w, float* out);
  void det_postprocess(const float* pred, int h, int w, int ori_h, int ori_w, float* boxes, float* scores, int max_out,
                       int* n_out);
  // form 0: pp::warp_crops (one grid row per crop), 1: pp::warp_crops_flat (rt_debug_warp_crops compares the two)
  void crop_images(const uint8_t* rgb, int h, int w, const float* boxes, int n, uint8_t* out, size_t out_cap, int form = 0);
  void resize_norm_image(const uint8_t* crop, int h, int w, int ori_h, int ori_w, int img_h, int img_w, float ratio,
                         float* out);
  void ctc_decode(const float* probs, int n, int t, int c, int32_t* idx, float* prob, int32_t* tokens,
                  int32_t* n_tokens, float* scores);
  // ---- the rec network's CTC tail (rec_tail.cpp) ----
  // What rec_tail reads and writes for ONE rec group, everything on the device: what every group has, then one member per kind,
  // left as it is where the plan has nothing of the kind.  Row and line arrays start at the group's first row / line; a kind's
  // per-line outputs are indexed by its Line::slot, the line's index in the call.
  // (rec_return_word_box, word_boxes.h: pp::word_boxes' arguments; h_lines: the group's descriptors in pinned memory; flip: the
  // lines' rec flip outcomes, rec_flip.h, or null)
  struct WordBoxes { const rt::pp::WordLineDesc* h_lines; const int* label; const float* cscore; int* cols; int* n_words; rt::wb::Word* words; const int* flip = nullptr; };
  struct RecTail {
    const float* z5 = nullptr;                // [rows, core.D] the head's input, inside a larger allocation (RecTailPlan::needs_z5)
    int* idx = nullptr; float* prob = nullptr;   // [rows] the fused head's argmax rows, in and out
    const rt::ImgGeom* lines = nullptr; int n_lines = 0;   // the token level: {first row, 1, T} per line
    int chunk_rows = 0;                       // rows per logits recompute (0: cc::CAND_CHUNK)
    int* tok = nullptr; int* ntok = nullptr; float* rscore = nullptr;   // pp::ctc_decode's outputs
    const WordBoxes* wb = nullptr;            // or null
    // rec charsets (ctc_charset.h): [.][words]
    struct Charsets { const uint32_t* masks = nullptr; int words = 0; } charsets;
    // rec lexicons (ctc_lexicon.h): lx::Tables on the device; loglik [plan.table], or null: taken from `scratch`; the per-line
    // matches [slot][lx::MATCHES] and counts.  Lexicon snap: the per-lexicon min_posterior and the per-line flags (both read and
    // written in a snap group only) and Viterbi values (optional)
    struct Lexicon {
      rt::lx::DevTables d{}; float* loglik = nullptr; rt::lx::Match* matches = nullptr; int* n = nullptr;
      const float* d_min_post = nullptr; int* snapped = nullptr; float* vit = nullptr;
    } lexicon;
    // rec patterns (ctc_pattern.h): pt::Tables on the device and the per-line results
    struct Pattern { rt::pt::DevTables d{}; int* matched = nullptr; float* vit = nullptr; float* logprob = nullptr; float* free_logprob = nullptr; } pattern;
    // rec keywords (ctc_keyword.h): the lists' lx::Tables and min_score on the device; score [plan.ktable] and span
    // [plan.ktable][2], or null: taken from `scratch`; the per-line hits [slot][kw::HITS] and counts
    struct Keywords {
      rt::lx::DevTables d{}; const float* d_min = nullptr; float* score = nullptr; int* span = nullptr; rt::kw::Hit* hits = nullptr; int* n = nullptr;
    } keywords;
    // rec beams (ctc_beam.h; b > 0 where the plan has beam lines): the width and the hypotheses per line; the per-line counts
    // [slot], records [slot][n] and the token pool (bm::Line::out)
    // fused: language-model fusion (ctc_lm.h) with fu, whose tables are on the device, and the records' lm / fused score [slot][n]
    struct Beam {
      int b = 0, n = 0; int* count = nullptr; rt::bm::Beam* recs = nullptr; int* tok = nullptr;
      bool fused = false; rt::lm::Fusion fu{}; rt::lm::BeamLm* lms = nullptr;
      // worded: the word-list constraint (ctc_vocab.h) with wc, whose tables are on the device, and the records' closed count /
      // closing score [slot][n]
      bool worded = false; rt::vc::Constraint wc{}; rt::vc::BeamVocab* vocs = nullptr;
    } beam;
    // rec_return_candidates = k > 0 (ctc_candidates.h): the kept tokens' time steps and [k] candidates
    struct Candidates { int k = 0; int* col = nullptr; rt::cc::Cand* cands = nullptr; } cand;
  };
  // The tail of one rec group behind the net, in the one order that is right: the charsets replace the restricted rows' (idx, prob)
  // before anything reads them; a snap group's lexicons run next, so that the decode reads the snapped lines' aligned rows;
  // then the patterns, whose matched lines overwrite theirs; pp::ctc_decode; the word boxes; any other group's lexicons; the
  // keywords and the beams, which read and write nothing of the others'; the candidates last, for their host wait.  The four
  // kinds of whole lines -- lexicons, patterns, keywords, beams -- share one pass (rec_tail.cpp LinePass): chunks of about
  // chunk_rows rows of whole lines, per chunk the row gather, the CTC FC, the row statistics, then the kind's own launches.  The
  // plan's tables go through `pinned` into `scratch`, where the workspace comes from too: the caller rewinds it per group, after this.
  void rec_tail(const rt::RecTailPlan& plan, const rt::SvtrCore& core, const RecTail& t);
  // rec_return_candidates = K (ctc_candidates.h): kept token j of a line at first row o gets col[o + j] and cands[(o + j) * K ...].
  // K > 1 waits for the stream once (the kept-row count sizes the logits GEMMs) and recomputes in chunks of kept rows.  d_row_set
  // (rec charsets, or null): a kept row r with d_row_set[r] = s >= 1 ranks the classes of set s only.
  void ctc_candidates(const rt::SvtrCore& core, const RecTail& t, long long rows, const int* d_row_set);
  // Rec charsets (ctc_charset.h): d_rows [n_rows] / d_row_set [rows] = the plan's crows / row_set.  In chunks of rows: row gather,
  // the CTC FC, k_ctc_charset_argmax, which overwrites idx / prob of exactly those rows.  No host wait.
  void ctc_charset(const rt::SvtrCore& core, const RecTail& t, const int* d_rows, int n_rows, const int* d_row_set);
  // Rec lexicons (ctc_lexicon.h) over the plan's lexicon lines, with k_ctc_row_lse: per chunk k_ctc_lexicon_forward -> loglik; then
  // one k_ctc_lexicon_topk over all lines -> matches / n.  No host wait.  A snap group (ctc_lexicon_align.h) runs the top-K per chunk,
  // then k_ctc_lexicon_align on the resident logits: it overwrites the snapped lines' rows of idx / prob and writes every snapped[slot].
  void ctc_lexicon(const rt::RecTailPlan& plan, const rt::SvtrCore& core, const RecTail& t);
  // Rec patterns (ctc_pattern.h) over the plan's pattern lines, with k_ctc_row_lse and k_ctc_row_max: per chunk
  // k_ctc_pattern_viterbi, which overwrites the matched lines' rows of idx / prob and writes every pattern line's results [slot].
  // No host wait.
  void ctc_pattern(const rt::RecTailPlan& plan, const rt::SvtrCore& core, const RecTail& t);
  // Rec keywords (ctc_keyword.h) over the plan's keyword lines, with k_ctc_row_max: per chunk k_ctc_keyword_spot -> score / span;
  // then one k_ctc_keyword_topk over all lines -> hits / n.  No host wait, and no value that anything else reads.
  void ctc_keywords(const rt::RecTailPlan& plan, const rt::SvtrCore& core, const RecTail& t);
  // Rec beams (ctc_beam.h) over the plan's beam lines, with k_ctc_row_lse: per chunk k_ctc_beam_topc, then k_ctc_beam_search on the
  // resident logits -> count / recs / tok.  The trie comes from `scratch`.  No host wait, and no value that anything else reads.
  void ctc_beams(const rt::RecTailPlan& plan, const rt::SvtrCore& core, const RecTail& t);
  // L2: one pipeline call over its pages, on this lane
  rt_results* run_pages(const PageCall& call);
};

// what a rule of rec_line_opts.h objects to, if anything
inline void rt_refuse(const std::string& why) { if (!why.empty()) throw rt::RtError(RT_ERR_INVALID, why); }

// The session: lane 0, and what the session owns once -- what every lane reads (config, device, networks, dictionary, rec
// stores), the defaults the setters write, the helper lanes with their host threads, the staging slots and the last error.
struct rt_session : rt_lane {
  rt_config cfg{};
  int device = 0;
  std::unique_ptr<rt::DetModel> det;
  std::unique_ptr<rt::ClsModel> cls;
  std::unique_ptr<rt::RecModel> rec;
  std::string model_info;
  std::vector<std::string> dict;  // RecCharacter (rec_processor.rs:29-46)
  // the rec charsets, lexicons, patterns and keyword lists, and how many of each there are: the valid ids
  std::unique_ptr<rt_charsets> charsets;
  std::unique_ptr<rt_lexicons> lexicons;
  std::unique_ptr<rt_patterns> patterns;
  std::unique_ptr<rt_keywords> keywords;
  std::unique_ptr<rt_lms> lms;
  std::unique_ptr<rt_vocabs> vocabs;
  rt::RecLineOpts rec_counts() const {
    return {(int)charsets->ids.size(), (int)lexicons->host.size(), (int)patterns->host.size(), (int)keywords->host.size()};
  }
  uint8_t* d_word_raw = nullptr;  // rec_return_word_box: wb::raw_class of every dictionary entry (device)
  // rt_set_rec_charset / _lexicon / _pattern / _keywords: the options of every line of the pipeline calls that follow, unless a region names
  // its own (0: none)
  rt::RecLineOpts rec_default;
  // rt_set_det_tiles (det_tiles.h): pages whose det input is larger than det_tile either way are detected in tiles; 0 = off
  int det_tile = 0, det_overlap = 0;
  // rt_set_rec_beam (ctc_beam.h): every line of the pipeline calls that follow also reports its beam_n most probable strings from
  // a prefix beam search of width beam_b; 0 = off
  int beam_b = 0, beam_n = 0;
  // rt_set_rec_beam_lm (ctc_lm.h): the beam search of the calls that follow ranks by total + (alpha * lm + beta * len) under
  // model beam_lm; -1 = off.  Without effect while beam_b = 0
  int beam_lm = -1; float lm_alpha = 0.0f, lm_beta = 0.0f;
  // rt_set_rec_beam_vocab (ctc_vocab.h): the beam search of the calls that follow charges every word of a hypothesis that is not
  // in vocabulary beam_vocab with vocab_gamma; -1 = off.  Without effect while beam_b = 0
  int beam_vocab = -1; float vocab_gamma = 0.0f;
  // rt_set_rec_windows (rec_windows.h): lines at least 8 columns wider than rec_window are read as overlapping windows whose
  // trusted time steps are stitched into the line's rows; 0 = off
  int rec_window = 0, rec_overlap = 0;
  // rt_set_rec_flip (rec_flip.h): lines whose classifier score is below rec_flip_below are read both ways up and the reading
  // with the better greedy CTC score is kept; 0 = off.  In (0, 1] every call syncs its lane once more, for the scores
  float rec_flip_below = 0.0f;
  CallSettings settings() const {
    return {rec_default, det_tile, det_overlap, beam_b, beam_n, rec_window, rec_overlap, beam_lm, lm_alpha, lm_beta, beam_vocab, vocab_gamma,
            rec_flip_below};
  }
  std::string last_error;
  // rt_charset_create: compiles the set (rt::compile_charset), stores it and returns its id
  int charset_create(const char* utf8, size_t len, const int32_t* ids, int n_ids);
  // rt_lexicon_create: the entries into the lexicon store (rt_entry_store::add); returns the lexicon's id
  int lexicon_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries);
  // rt_keywords_create: the entries into the keyword store (rt_entry_store::add) with min_score; returns the list's id
  int keywords_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries, float min_score);
  // rt_lm_create: compiles the ARPA text (rt::lm::compile_arpa over the dictionary), stores the model and returns its handle
  int lm_create(const char* arpa, size_t len, float oov_log10);
  // rt_vocab_create: compiles the words (rt::compile_vocab over the dictionary), stores the vocabulary and returns its handle
  int vocab_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens, int n_id_words, int flags);
  // rt_pattern_create: compiles the pattern (rt::pt::compile), stores it and returns its id
  int pattern_create(const char* utf8, size_t len);
  // rt_lexicon_set_snap: the lexicon's min_posterior (ctc_lexicon_align.h), on the host and in the device table
  void lexicon_set_snap(int lexicon, float min_posterior);
  // rt_debug_det_tiles: the det stage of a one-page call on a host RGB8 image at det-input size h x w, through the pipeline's own
  // det_groups under the session's det tiles; tile_maps_out: every tile's own map packed in plan order, page_map_out [h * w]
  void debug_det_tiles(const uint8_t* rgb_det, int h, int w, float* tile_maps_out, float* page_map_out);
  // rt_debug_rec_windows: n lines of [3, 48, widths[i]] (host, NCHW, concatenated) as ONE rec group through the pipeline's own
  // cut, network and stitch (rec_group_net) under the session's rec windows.  Every output is optional and on the host: the
  // units' rows in unit order, line after line (idx / prob [unit rows], z5 [unit rows][120]), and the lines' stitched rows
  void debug_rec_windows(const float* nchw, int n, const int* widths, int32_t* unit_idx_out, float* unit_prob_out, float* unit_z5_out,
                         int32_t* line_idx_out, float* line_prob_out, float* line_z5_out);
  // rt_debug_rec_flip: n RGB8 crops (host, packed back to back, hw[2 i] x hw[2 i + 1] pixels) as ONE rec group through the
  // pipeline's own rotate, resize_norm, network, score and select (rec_group_flip) at the padded width of max_wh_ratio, under
  // the session's rec windows; both[i] != 0: line i is read both ways.  Every output is optional and on the host
  struct RecFlipOut {
    int32_t* view_idx = nullptr; float* view_prob = nullptr;     // [views][T]: the n lines' view 0, then the flagged lines' view 1
    float* view_z5 = nullptr;                                    // [views][T][120]
    int32_t* view_ntok = nullptr; float* view_score = nullptr;   // [views]
    int32_t* taken = nullptr;                                    // [n]: 1 where view 1 was taken
    int32_t* idx = nullptr; float* prob = nullptr; float* z5 = nullptr;   // [n][T] (z5: [n][T][120]) the lines' final rows
  };
  void debug_rec_flip(const uint8_t* crops, const int* hw, int n, const uint8_t* both, float max_wh_ratio, const RecFlipOut& out);

  // ---- lanes, tickets, staging (session_batch.cpp) ----
  // extra lanes: own stream / arenas; rt_run_batch splits the pages over the lanes and runs them on concurrent host threads
  std::vector<std::unique_ptr<rt_lane>> helpers;
  int n_lanes() const { return (int)helpers.size() + 1; }
  rt_lane* lane(int l) { return l == 0 ? this : helpers[(size_t)l - 1].get(); }
  int active_lanes = 1 << 30;  // rt_set_lanes: upper bound on the lanes rt_run_batch uses
  int lanes_for(int n_pages) const { return rt::lanes_for(n_lanes(), active_lanes, n_pages); }
  // persistent lane threads (one per lane) and the number of submitted, not yet waited batches
  std::vector<std::unique_ptr<LaneWorker>> workers;
  std::atomic<int> inflight{0};
  int next_lane = 0;               // first lane of the next submitted batch
  // page staging: host pages of a submitted batch are copied to HBM by the submitting thread on a copy stream of their own, one
  // batch ahead of the lanes that read them (slots are reused; one per batch in flight)
  struct StageSlot { uint8_t* p = nullptr; size_t cap = 0; std::vector<hipEvent_t> ev; bool busy = false; };
  std::vector<StageSlot> stage_slots;
  hipStream_t st_copy = nullptr;
  int acquire_slot(size_t bytes, int nl);  // a free slot of at least `bytes` with nl events (-1: out of device memory)
  void stage_pages(rt_ticket* t);          // picks the slot
  void stage_part(rt_ticket* t, int l);    // copies the pages of lane part l
  void release_stage(rt_ticket* t);
  void free_stage();
  void ensure_workers();
  // a pipeline call over the caller's arrays under the session's settings as they are now
  PageCall call_of(const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem, const float* const* det_map_override = nullptr,
                   rt_stage_callback cb = nullptr, void* user = nullptr) const {
    return PageCall{n_pages, mem, rgb, hs, ws, det_map_override, nullptr, nullptr, nullptr, settings(), cb, user};
  }
  // the call's pages split over the lanes and queued on their threads; enc: the call's pages are these, still encoded
  rt_ticket* submit_batch(const PageCall& call, std::vector<rt::EncodedPage>* enc = nullptr);
  rt_results* wait_batch(rt_ticket* t);   // consumes the ticket
  // a call that takes one lane: on the caller's thread, lane 0 (no hand-over in the single-page latency path)
  rt_results* run_on_caller(const PageCall& call);
  rt_results* run_batch(const PageCall& call);
  // rt_decode_batch: pages through the host stage and the reconstruction kernels into out[i] (mem: RT_MEM_HOST / RT_MEM_DEVICE)
  void decode_batch(std::vector<rt::EncodedPage>& enc, uint8_t* const* out, int mem);
  // rt_run_regions: checks and clamps every quad (RT_ERR_INVALID naming page and region; nothing is queued then), then the
  // pages go over the lanes as run_batch's do, from the crop plan on
  // ids[j] (the kinds of rec_line_opts.h: charsets, lexicons, patterns, keywords; each or null; entries may be null): per region
  // -1 = the session default, 0 = none, >= 1 = that id (rt::resolve_region_opts); a region may not carry both a pattern and a lexicon
  rt_results* run_regions(const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                          const float* const* quads, const int* n_quads, const int* const* const ids[rt::REC_N_KINDS]);
};

rt_session* rt_session_create(const rt_config* cfg);
std::string rt_format_f32_impl(float v);  // serde_json / ryu form of an f32
namespace rt {
// (the three below live in rec_tail.cpp)
// RecCharacter::new (rec_processor.rs:29-46) with Rust's from_utf8 / lines / trim semantics
std::vector<std::string> load_dictionary(const std::vector<uint8_t>& bytes);
// A rec charset (ctc_charset.h) as its mask of cs::mask_words(dict.size()) words: the blank, every dictionary class whose whole
// entry is one code point of utf8 [len] (duplicates all join; U+0020 is the appended " "), and ids [n_ids].  Throws RT_ERR_UTF8
// for malformed text, RT_ERR_INVALID for a code point that matches no entry ("U+XXXX") or an id outside [0, dict.size()).
std::vector<uint32_t> compile_charset(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids,
                                      int n_ids);
// A rec lexicon (ctc_lexicon.h) as flat class ids and one length per entry: the lines of utf8 [len] (split and trimmed as the
// dictionary's lines are; empty lines skipped), each code point the LOWEST class id whose whole dictionary entry is that code
// point (U+0020 is the appended " "), then n_id_entries entries of entry_lens[i] ids each, consecutive in ids.  Throws RT_ERR_UTF8
// for malformed text; RT_ERR_INVALID for a code point that matches no entry ("U+XXXX", naming the entry), an id outside
// [1, dict.size()), an empty id entry, an entry longer than lx::MAX_LEN, or no entry at all; RT_ERR_CAPACITY past lx::MAX_ENTRIES.
void compile_lexicon(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids,
                     const int32_t* entry_lens, int n_id_entries, std::vector<int32_t>& ids_out, std::vector<int32_t>& lens_out);
// A vocabulary's words (ctc_vocab.h) in their id form: the lines of utf8 [len], split, trimmed and mapped as compile_lexicon maps
// them -- with flags & vc::CASE_VARIANTS each followed by the word with its first ASCII letter upper-cased and the word with all
// of them upper-cased, a variant with a code point the dictionary lacks being left out and counted -- then n_id_words words of
// word_lens[i] ids each.  A word already there is not added again.  Throws RT_ERR_UTF8 for malformed text; RT_ERR_INVALID, naming
// the word, for a code point that matches no entry ("U+XXXX"), the blank or an id outside [1, dict.size()), an empty or over-long
// word, no word at all, unknown flag bits; RT_ERR_CAPACITY past vc::MAX_WORDS.  The second form also compiles it (vc::compile).
void compile_vocab(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens,
                   int n_id_words, int flags, vc::Ids& out, int* variants_dropped);
vc::Vocab compile_vocab(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens,
                        int n_id_words, int flags, vc::Ids& f);
}

// Launchers of the pre/post-processing kernels (prepost_kernels.hip): everything in
// retto-core's DetProcessor / ClsProcessor / RecProcessor / ImageHelper that is not a
// network forward.  Bit-exact integer / f32 / f64 arithmetic (no FMA contraction).
#pragma once
#include "nn.h"
#include "common.h"
#include "word_boxes.h"
#include "ctc_beam.h"
#include "ctc_candidates.h"
#include "ctc_charset.h"
#include "ctc_keyword.h"
#include "ctc_lexicon.h"
#include "ctc_lexicon_align.h"
#include "ctc_pattern.h"
#include "det_tiles.h"
#include "rec_windows.h"
#include "rec_flip.h"

namespace rt {
namespace pp {

// image 0.25.6 imageops::thumbnail on RGB8 (used by image_helper.rs:124,139,168,184)
void thumbnail_rgb8(hipStream_t st, const uint8_t* src, int h, int w, uint8_t* dst, int nh, int nw, int* err_flag);

// det_processor.rs:151-160 + image_helper.rs:211-221: RGB8 HWC -> normalised BGR f32.
// layout 0: NHWC pitch 4 (B,G,R,0); layout 1: CHW planes
void det_normalize(hipStream_t st, const uint8_t* rgb, int h, int w, float scale, const float* mean3,
                   const float* std3, int layout, float* out);

// ---- DB post-processing (det_processor.rs:279-335) -------------------------------
struct DbParams {
  float thresh, box_thresh, unclip_ratio;
  int min_size, dilate;
  int score_mode;   // rt_config.det_score_mode: 0 = Fast (min-area rect), 1 = Slow (the contour's own polygon)
};
struct DbBox { float pts[8]; float score; int key; };
// Work buffers for one page of H x W; sized by db_workspace_bytes() (score_mode 1 adds the Slow kernels' buffers).
size_t db_workspace_bytes(int H, int W, int max_boxes, int score_mode);
struct DbPageIn { const float* pred; int H, W, ori_h, ori_w; };
size_t db_page_desc_bytes();
// Runs the whole post-process for n pages with shared launches (blockIdx.y = page).
// workspaces[i]: device buffer of db_workspace_bytes(H_i, W_i, max_boxes, p.score_mode); boxes_out[i]
// (device, max_boxes entries) receives the sorted boxes in after_* coordinates,
// count_out[i][0] the number, count_out[i][1] != 0 signals a capacity overflow.
// h_desc (pinned host) / d_desc (device): n * db_page_desc_bytes() scratch for the page table.
void db_postprocess_batch(hipStream_t st, int n, const DbPageIn* in, const DbParams& p, void* const* workspaces,
                          int max_boxes, DbBox* const* boxes_out, int* const* count_out, void* h_desc, void* d_desc);
// boxes [n][max_boxes] + counts [n][2] (both contiguous over the pages) -> packed list in page order
void pack_boxes(hipStream_t st, int n, const DbBox* boxes, const int* counts, int max_boxes, DbBox* packed);

// ---- crops -------------------------------------------------------------------------
struct CropDesc {
  const uint8_t* src; int sh, sw;   // source page (after resize_both)
  float inv[9];                     // output pixel -> source pixel
  int w, h, rot;                    // pre-rotation dims, rotate270 flag
  long long out_off;                // byte offset of this crop in the crop pool
  long long pix_base;               // output pixels (w * h) of the crops before this one: warp_crops_flat's work list
};
// one grid row per crop, each as long as the largest crop (max_pix): the launch for crops of about one size
void warp_crops(hipStream_t st, const CropDesc* descs, int n, int max_pix, uint8_t* pool);
// the same crops, byte for byte, walked as one flat list of total_pix = sum of w * h output pixels: ceil(total_pix / 256)
// workgroups, at most WARP_FLAT_MAX_BLOCKS, which stride over the rest.  A thread finds its crop by binary search over pix_base.
constexpr int WARP_FLAT_MAX_BLOCKS = 16384;
void warp_crops_flat(hipStream_t st, const CropDesc* descs, int n, long long total_pix, uint8_t* pool);

// cls_processor.rs:108-121,163-166: argmax of [n,2]; rotate180 in place when label==180 && score>=thresh
struct CropRef { long long off; int h, w; int pad_; };   // final (post-rotation) dims
void cls_post_rotate(hipStream_t st, const float* probs, const int* crop_of_row, int rows, float thresh,
                     const CropRef* crops, uint8_t* pool, int max_pix, int* label_idx, float* score);

// image_helper.rs:176-209 resize_norm_image for a ragged batch of lines.
struct LineDesc {
  long long crop_off; int h, w;   // crop in the pool (current dims)
  int resized_w, W;               // thumbnail width, padded width
  long long out_off;              // element offset of this line's tensor in `out`
};
// layout 0: NHWC pitch 4 (R,G,B,0) per line [img_h][W][4]; layout 1: CHW [3][img_h][W]
void resize_norm(hipStream_t st, const LineDesc* lines, int n, int img_h, int max_W, const uint8_t* pool, int layout,
                 float* out, int* err_flag);

// rec_processor.rs:48-97 CTC greedy decode over per-token (argmax, prob) rows.
// tok_off[i] = first row of line i, T[i] rows; tokens written compacted at the same offsets.
void ctc_decode(hipStream_t st, const int* idx, const float* prob, const ImgGeom* lines, int n, int* tokens,
                int* n_tokens, float* score);

// rt_config.rec_return_word_box: the words of n lines of one rec group (word_boxes.h), one wave64 per line.  idx: the group's
// argmax rows; tokens / n_tokens: what ctc_decode wrote for the same lines; label / cls_score: the lines' cls results (the
// rotate180 predicate of cls_post_rotate); flip: the lines' rec flip outcomes (rec_flip.h: a taken view 1 inverts rot180), or
// null; raw_of_id: the session's class table.  Per line i: word count -> n_words[i], words
// -> words[tok_off ...] (a line has at most as many words as kept tokens); cols: scratch of the group's token count.
struct WordLineDesc { long long tok_off; wb::WordGeom g; };   // tok_off: first argmax row of the line inside the group
void word_boxes(hipStream_t st, const int* idx, const int* tokens, const int* n_tokens, const int* label, const float* cls_score,
                float cls_thresh, const int* flip, const uint8_t* raw_of_id, const WordLineDesc* lines, int n, int* cols,
                int* n_words, wb::Word* words);

// rt_config.rec_return_candidates (ctc_candidates.h) over the n lines of one rec group; lines[i] = {first row, 1, T_i}, what
// ctc_decode got.  kept_rows: one wave64 per line writes, at the line's row offset, the kept time steps -> cols and rank 0
// (idx, prob at the step) -> cands[slot * K]; with kept_row / kept_slot (K > 1) also the group's compact list of kept rows and
// their token slots, in line order (line i starts at the sum of n_tokens[0..i), ctc_decode's counts), and the list's length ->
// *n_kept.
void ctc_kept_rows(hipStream_t st, const int* idx, const float* prob, const ImgGeom* lines, const int* n_tokens, int n, int K,
                   int* cols, cc::Cand* cands, int* kept_row, int* kept_slot, int* n_kept);
// rows kept_row[0..m) of z [.][ld] (ld a multiple of 4) -> out [m][ld]
void ctc_gather_rows(hipStream_t st, const float* z, int ld, const int* kept_row, int m, float* out);
// one wave64 per row i < m of logits [m][ld]: ranks 1..K-1 over the columns [0, classes) other than cands[kept_slot[i] * K].id
// -> cands[kept_slot[i] * K + 1 ...].  With kept_row / row_set / masks (rec charsets, ctc_charset.h): row i is time step
// kept_row[i] of the group, and where row_set[kept_row[i]] = s >= 1 only the classes of masks[(s - 1) * words ...] take part.
void ctc_topk(hipStream_t st, const float* logits, int ld, int classes, const int* kept_slot, int m, int K, cc::Cand* cands,
              const int* kept_row = nullptr, const int* row_set = nullptr, const uint32_t* masks = nullptr, int words = 0);
// Rec charsets (ctc_charset.h): one wave64 per row i < m of logits [m][ld], time step rows[i] of the group with charset
// row_set[rows[i]] = s >= 1: the argmax and its probability over the classes of masks[(s - 1) * words ...] -> idx[rows[i]],
// prob[rows[i]].  masks: [n_sets][words = cs::mask_words(classes)] on the device.
void ctc_charset_argmax(hipStream_t st, const float* logits, int ld, int classes, const int* rows, const int* row_set,
                        const uint32_t* masks, int words, int m, int* idx, float* prob);
// Rec lexicons (ctc_lexicon.h): one wave64 per row i < m of logits [m][ld]: lse[i] = log-sum-exp over the columns < classes
void ctc_row_lse(hipStream_t st, const float* logits, int ld, int classes, int m, float* lse);
// The CTC forward log-likelihood of every entry of the lexicon of each of lines[0..n_lines) (one chunk: their rows are resident
// in logits [.][ld] and lse, row r of the call's compact row list at r - chunk_row0) -> loglik[line.out + entry], -inf where the
// entry is infeasible for the line's T.  max_waves: the largest lx::waves_of over the lexicons of these lines.  lex / entries /
// order / ids: lx::Tables on the device.
void ctc_lexicon_forward(hipStream_t st, const float* logits, int ld, const float* lse, const lx::Line* lines, int n_lines,
                         int chunk_row0, int max_waves, const lx::Lex* lex, const lx::Entry* entries, const int* order,
                         const int* ids, float* loglik);
// one wave64 per line over its loglik row: up to lx::MATCHES matches -> matches[line.slot * lx::MATCHES ...], their number ->
// counts[line.slot] (slots of a line's row past its count are not written)
void ctc_lexicon_topk(hipStream_t st, const lx::Line* lines, int n_lines, const lx::Lex* lex, const float* loglik,
                      lx::Match* matches, int* counts);
// Rec keywords (ctc_keyword.h): every entry of the keyword list of each of lines[0..n_lines) spotted inside the line (one chunk,
// resident as for ctc_lexicon_forward, with rmax of its rows: ctc_row_max) -> score[line.out + entry] and span[2 * (line.out +
// entry) ..] = its first and last column; -inf and (-1, -1) where the entry is infeasible for the line's T.  max_waves: the
// largest lx::waves_of over the lists of these lines.  lex / entries / order / ids: the lists' lx::Tables on the device.
void ctc_keyword_spot(hipStream_t st, const float* logits, int ld, const float* rmax, const kw::Line* lines, int n_lines,
                      int chunk_row0, int max_waves, const lx::Lex* lex, const lx::Entry* entries, const int* order, const int* ids,
                      float* score, int* span);
// one wave64 per line over its score row: up to kw::HITS hits that pass min_score[line.lex] -> hits[line.slot * kw::HITS ...]
// (entry, score, first_col, last_col; never the quad), their number -> counts[line.slot] (slots past the count are not written)
void ctc_keyword_topk(hipStream_t st, const kw::Line* lines, int n_lines, const lx::Lex* lex, const float* min_score,
                      const float* score, const int* span, kw::Hit* hits, int* counts);
// Rec beams (ctc_beam.h): K_t of every row i < m of logits [m][ld] -> topc[i]
void ctc_beam_topc(hipStream_t st, const float* logits, int ld, int classes, int m, bm::TopC* topc);
// the prefix beam search of lines[0..n_lines) (one chunk, resident as for ctc_lexicon_forward, with lse and topc of its rows:
// ctc_row_lse, ctc_beam_topc), beam width B, nbest hypotheses: counts[line.slot] <- their number, beams[line.slot * nbest ...]
// their records, tokens[line.out + k * T ...] hypothesis k's tokens (slots past a count or a length are not written).  nodes: the
// group's trie, bm::nodes_of(T, B) nodes per line from line.lex on; needs no initialisation.
void ctc_beam_search(hipStream_t st, const float* logits, int ld, const float* lse, const bm::TopC* topc, const bm::Line* lines,
                     int n_lines, int chunk_row0, int B, int nbest, bm::Node* nodes, bm::Beam* beams, int* tokens, int* counts,
                     const lm::Fusion* fu = nullptr, lm::BeamLm* lms = nullptr, const vc::Constraint* wc = nullptr,
                     vc::BeamVocab* vocs = nullptr);
// Lexicon snap (ctc_lexicon_align.h): one wave64 per line of lines[0..n_lines) (one chunk, resident as for ctc_lexicon_forward,
// after ctc_lexicon_topk over the same lines).  snapped[line.slot] <- 0 / 1 for every line; a line whose lexicon has
// min_post[line.lex] > 0 and whose match 0 reaches it has its winner aligned (CTC Viterbi) and its rows rows[line.row0 ..
// + T) of idx / prob overwritten by the path; vit (optional): the end state's Viterbi value -> vit[line.slot], snapped lines
// only.  bp: 16 bytes per row of the chunk (16-byte aligned), the backpointers of the lines longer than la::TILE steps.
void ctc_lexicon_align(hipStream_t st, const float* logits, int ld, const float* lse, const lx::Line* lines, int n_lines,
                       int chunk_row0, const lx::Lex* lex, const lx::Entry* entries, const int* ids, const float* min_post,
                       const lx::Match* matches, const int* counts, const int* rows, void* bp, int* idx, float* prob, int* snapped,
                       float* vit);
// Rec patterns (ctc_pattern.h): one wave64 per row i < m of logits [m][ld]: rmax[i] = the largest logit of the columns < classes
void ctc_row_max(hipStream_t st, const float* logits, int ld, int classes, int m, float* rmax);
// The pattern Viterbi: one workgroup per line of lines[0..n_lines) (one chunk, resident as for ctc_lexicon_forward, with lse and
// rmax of its rows).  Per line matched / vit / logprob / free_lp [line.slot]; a matched line's rows rows[line.row0 .. + T) of
// idx / prob are overwritten by the path.  tb: pt::Tables on the device.  bp: the chunk's backpointer codes (16 bits each,
// line.bp counts in codes), read and written only for lines with pt::bp_codes(T, P, S) > pt::BP_LDS.
void ctc_pattern_viterbi(hipStream_t st, const float* logits, int ld, int classes, const float* lse, const float* rmax,
                         const pt::Line* lines, int n_lines, int chunk_row0, const pt::DevTables& tb, const int* rows, void* bp,
                         int* idx, float* prob, int* matched, float* vit, float* logprob, float* free_lp);

// sum of a float buffer into per-block doubles (partials has ceil(n/65536) entries)
int sum_blocks(long long n);
void sum_partial(hipStream_t st, const float* x, long long n, double* partials);

// det tiles (det_tiles.h), one launch per det group each over the group's n tiles (tiles: device; max_tile_pix: the largest
// th * tw).  cut: every tile's pixels out of its page's RGB8 det image, contiguous at cut + cut_off (16-byte aligned), the form
// DetModel::run_u8 reads.  stitch: every tile's owned rectangle from maps + map_off into its page map.
void det_tile_cut(hipStream_t st, const dt::TileDesc* tiles, int n, long long max_tile_pix, uint8_t* cut);
void det_tile_stitch(hipStream_t st, const dt::TileDesc* tiles, int n, long long max_tile_pix, const float* maps);

// rec windows (rec_windows.h), one launch per windowed rec group each over the group's n units (units: device; max_w: the widest
// unit's columns, max_rows: the most steps a unit owns).  cut: lines = the group's line tensors as resize_norm wrote them, unit
// = the ragged unit tensors, both NHWC-4 of h rows.  stitch: the owned rows of the units' idx / prob / z5 (z5 [rows][120], or
// null with line_z5 null) into the line rows.
void rec_window_cut(hipStream_t st, const rw::UnitDesc* units, int n, int h, int max_w, const float* lines, float* unit);
void rec_window_stitch(hipStream_t st, const rw::UnitDesc* units, int n, int max_rows, const int* unit_idx, const float* unit_prob,
                       const float* unit_z5, int* line_idx, float* line_prob, float* line_z5);

// rec flip (rec_flip.h), one launch per rec group with a both-ways line each.  rotate: the n flagged crops (crops: device) as one
// flat list of total_pix pixels, crop c from pool + src_off rotated by 180 degrees to flipped + dst_off.  select: per both-ways
// line (lines: device, n of them, max_T the most time steps of one) the choice between its two views from ctc_decode's v_ntok /
// v_score over the views, -> outcome[slot] (rf::KEPT_0 / TOOK_1) and scores[2 slot ...]; the chosen view's rows of v_idx /
// v_prob -> idx / prob, and a taken view 1's z5 rows over the line's rows INSIDE v_z5 (or null), whose prefix the lines' z5 is.
void rec_flip_rotate(hipStream_t st, const rf::FlipCrop* crops, int n, long long total_pix, const uint8_t* pool, uint8_t* flipped);
void rec_flip_select(hipStream_t st, const rf::SelectDesc* lines, int n, int max_T, const int* v_ntok, const float* v_score,
                     const int* v_idx, const float* v_prob, float* v_z5, int* idx, float* prob, int* outcome, float* scores);

}  // namespace pp
}  // namespace rt

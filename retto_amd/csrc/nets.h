// The three networks behind RettoInnerWorker::{det,cls,rec}
// (/root/reference/retto-core/src/worker.rs:69-73), built from RTWB blobs and run as
// sequences of nn:: kernel launches over ragged NHWC batches.  Architecture: PP-OCRv4
// mobile det (PPLCNetV3 x0.75 + RSEFPN + DBHead), ch_ppocr_mobile_v2.0 cls
// (MobileNetV3-small x0.35) and PP-OCRv4 rec (PPLCNetV3 x0.95 + SVTR neck + CTC head);
// see SURVEY.md Appendix C.
#pragma once
#include <memory>
#include <string>
#include <map>
#include <vector>

#include "nn.h"
#include "runtime.h"

namespace rt {

// A pyramid level of a ragged batch: host copy + device copy of the per-image geometry.
struct Level {
  std::vector<ImgGeom> h;
  const ImgGeom* d = nullptr;
  long long total = 0;    // pixels over all images
  int maxH = 0, maxW = 0;
  long long maxPix = 0;   // max H*W over images
  int n() const { return (int)h.size(); }
  // row tile -> image tables of the SE-scaled GEMMs (nets.cpp run_lc), by tile height: built and uploaded once per pass
  mutable std::map<int, const int*> a_tabs;
};

struct RunCtx {
  hipStream_t st;
  Arena* arena;     // activations + descriptor tables of this pass
  Pinned* pinned;   // host staging for descriptor uploads
  Profiler* prof;
};

Level make_level(const std::vector<std::pair<int, int>>& hw);
Level flat_level(const Level& in);                             // one "image" of 1 x total pixels: a 1x1 conv as a GEMM over rows
Level down_level(const Level& in, int sh, int sw);             // conv k odd, pad k/2
Level pool_level(const Level& in, int kh, int kw);             // stride = kernel, no pad
void upload_levels(RunCtx& c, std::vector<Level*> levels);     // one H2D copy for all tables

struct PackedDense {  // gemm / conv_sp weights on device
  float* w = nullptr; float* b = nullptr;
  int K = 0, N = 0, Npad = 0, kh = 1, kw = 1;
};
struct PackedDw { float* w = nullptr; float* b = nullptr; int k = 3, C = 0, Cp = 0; };
struct Lab { int has = 0; float a = 1.f, c = 0.f; };
struct SeW { float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr; int C = 0, Cr = 0; };

class WeightStore {  // owns one device allocation per network
 public:
  ~WeightStore();
  float* upload(const std::vector<float>& host);
  void* upload_bytes(const void* host, size_t bytes);
  size_t bytes() const { return total_; }
 private:
  std::vector<void*> bufs_;
  size_t total_ = 0;
};

PackedDense pack_conv(WeightStore& ws, const Blob& b, const std::string& name, int cout, int cin, int kh, int kw);
PackedDense pack_conv(WeightStore& ws, const float* w, const float* bias, int cout, int cin, int kh, int kw);   // host w [cout][cin][kh][kw], bias [cout] or null
PackedDw pack_dw(WeightStore& ws, const float* w, const float* bias, int C, int k);   // host w [C][k][k] (torch depthwise layout), bias [C]
PackedDense pack_linear(WeightStore& ws, const Blob& b, const std::string& name, int cin, int cout);
PackedDense pack_linear(WeightStore& ws, const float* w, const float* bias, int cin, int cout);   // host w [cin][cout], bias [cout] or null
float* upload_raw(WeightStore& ws, const Blob& b, const std::string& name, size_t expect_numel);
void pack_stem(WeightStore& ws, const float* w, const float* bias, int cout, float** w_out, float** b_out);   // host w [cout][3][3][3], bias [cout] -> [27][cout], [cout]
SeW get_se(WeightStore& ws, const float* w1, const float* b1, const float* w2, const float* b2, int C, int Cr);   // host fc1 w [Cr][C], b [Cr], fc2 w [C][Cr], b [C]
// Host-side operands of the upsampling-aware FPN convs (nn_fpn.hip) from a raw 3x3 conv weight w [24][cin_total][3][3]; DetNet's
// constructor and rt_debug_fpn call the same functions (layouts: at their definitions in nets.cpp).
std::vector<float> fpn_fine_weights(const float* w, int cin_total, int c0, int cc, int cf);   // [9 taps][24 n][cf]
std::vector<float> fpn_phase_weights(const float* w, int cin_total, int c0, int cc);          // [cc / 24][4 phases][4 taps][24 n][24 k]
std::vector<float> fpn_class_weights(const float* w, int cin_total, int c0);                  // [9 classes][9 taps][24 n][24 k]
std::vector<float> fpn_lateral_weights(const float* w, int cin, int C);                       // 1x1 lateral w [C][cin] -> [cin][C]
std::vector<float> fpn_tap_weights(const float* w, int C);                                    // w [24][C][3][3] -> [9 taps][24 n][C m]
// Row-block table of the squeeze-excite-scaled GEMMs (Epilogue::a_tab) over the images of a level, for blocks of tile_rows = 128
// (2 ints per block) or 256 (3 ints per block, k_gemm32p): se_row_table_len(total, tile_rows) ints.
size_t se_row_table_len(long long total, int tile_rows);
void se_row_table(const std::vector<ImgGeom>& imgs, long long total, int tile_rows, int* tab);
// Line-boundary flags of the flat token list nn::conv13_flat runs over: flags[rows], bit 0 = first token of its line, bit 1 = last
// (lines = the H = 1 images of a token level; a line without tokens sets nothing).
void token_line_flags(const std::vector<ImgGeom>& lines, long long rows, unsigned char* flags);
Epilogue make_epi(const PackedDense& p, int act, const Lab* lab = nullptr, const float* residual = nullptr, int ld_res = 0);

struct LcBlock {
  PackedDw dw; Lab dw_lab; int dw_act = 0;
  bool se = false; SeW sew;
  PackedDense pw; Lab pw_lab;
  int sh = 1, sw = 1, cin = 0, cout = 0;
};

// The block on the kernels of its plan (nn::lc_plan for its shape on level Lout): x at Lin -> the block's output at Lout, pitch
// chan_pitch(b.cout).  y = null: arena memory; y1: the depthwise output where the plan's route is nn::LC_UNFUSED (null: arena
// memory; a GEMM tile reads rows past its end, which a caller's buffer must hold).
// trace (diagnostics, rt_debug_lc_wide): what the unfused route did -- nothing it launches or allocates depends on it.
struct LcTrace {
  const float* scale = nullptr;   // the squeeze-excite scales [image][Cp] (arena memory), where the block has them
  bool scaled_in_place = false;   // run_se multiplied them into y1; false: folded into the GEMM (or no squeeze-excite)
  nn::GemmPlan gemm;              // the pointwise GEMM's plan
};
nn::LcPlan lc_block_plan(const LcBlock& b, const Level& Lout);
float* run_lc(RunCtx& c, const LcBlock& b, const float* x, const Level& Lin, const Level& Lout, float* y = nullptr, float* y1 = nullptr,
              LcTrace* trace = nullptr);

// The blocks of the three mobile networks (fp32 and fp16 builds of the same graphs)
struct LcSpec { const char* name; int k, cin, cout, sh, sw; bool se; };
inline constexpr LcSpec DET_SPEC[] = {
    {"s2.0", 3, 16, 32, 1, 1, false}, {"s3.0", 3, 32, 48, 2, 2, false}, {"s3.1", 3, 48, 48, 1, 1, false},
    {"s4.0", 3, 48, 96, 2, 2, false}, {"s4.1", 3, 96, 96, 1, 1, false}, {"s5.0", 3, 96, 192, 2, 2, false},
    {"s5.1", 5, 192, 192, 1, 1, false}, {"s5.2", 5, 192, 192, 1, 1, false}, {"s5.3", 5, 192, 192, 1, 1, false},
    {"s5.4", 5, 192, 192, 1, 1, false}, {"s6.0", 5, 192, 384, 2, 2, true}, {"s6.1", 5, 384, 384, 1, 1, true},
    {"s6.2", 5, 384, 384, 1, 1, false}, {"s6.3", 5, 384, 384, 1, 1, false}};
inline constexpr LcSpec REC_SPEC[] = {
    {"s2.0", 3, 16, 32, 1, 1, false}, {"s3.0", 3, 32, 64, 1, 1, false}, {"s3.1", 3, 64, 64, 1, 1, false},
    {"s4.0", 3, 64, 128, 2, 1, false}, {"s4.1", 3, 128, 128, 1, 1, false}, {"s5.0", 3, 128, 240, 1, 2, false},
    {"s5.1", 5, 240, 240, 1, 1, false}, {"s5.2", 5, 240, 240, 1, 1, false}, {"s5.3", 5, 240, 240, 1, 1, false},
    {"s5.4", 5, 240, 240, 1, 1, false}, {"s6.0", 5, 240, 480, 2, 1, true}, {"s6.1", 5, 480, 480, 1, 1, true},
    {"s6.2", 5, 480, 480, 2, 1, false}, {"s6.3", 5, 480, 480, 1, 1, false}};
struct ClsSpec { int k, mid, cout; bool se; int act, sh, sw; };
inline constexpr ClsSpec CLS_SPEC[] = {
    {3, 8, 8, true, ACT_RELU, 2, 1},      {3, 24, 8, false, ACT_RELU, 2, 1},    {3, 32, 8, false, ACT_RELU, 1, 1},
    {5, 32, 16, true, ACT_HSWISH, 2, 1},  {5, 88, 16, true, ACT_HSWISH, 1, 1},  {5, 88, 16, true, ACT_HSWISH, 1, 1},
    {5, 40, 16, true, ACT_HSWISH, 1, 1},  {5, 48, 16, true, ACT_HSWISH, 1, 1},  {5, 104, 32, true, ACT_HSWISH, 2, 1},
    {5, 200, 32, true, ACT_HSWISH, 1, 1}, {5, 200, 32, true, ACT_HSWISH, 1, 1}};
// One MobileNetV3 block of the angle classifier: x at Lin (pitch cin) -> the block's output at Lout (pitch linear.N; y = null: arena
// memory).  One k_cls_block launch where cls_block_fused() says so (nn::g_cls_fused and nn::cls_block_supported), else the
// launch series expand GEMM -> depthwise -> run_se -> linear GEMM, whose GEMMs read rows past the end of x.
struct ClsBlock { PackedDense expand, linear; PackedDw dw; bool se = false; SeW sew; int act = ACT_RELU, sh = 1, sw = 1, cin = 0; bool shortcut = false; };
bool cls_block_fused(const ClsBlock& b, const Level& Lin, const Level& Lout);
float* run_cls_block(RunCtx& c, const ClsBlock& b, const float* x, const Level& Lin, const Level& Lout, float* y = nullptr);
Lab get_lab(const Blob& b, const std::string& name);   // the LearnableAffineBlock <name>.a / .c of a blob, where it has one

// The three worker functions as interfaces (RettoInnerWorker::{det,cls,rec}, worker.rs:69-73): the fp32 mobile
// networks below and the fp16 mobile / server networks of nets_f16.h implement them; the session only sees these.
class DetModel {
 public:
  virtual ~DetModel() {}
  // x: f32 NHWC pitch-4 (B,G,R,0) at level L0 (every H,W a multiple of 32).
  // Returns the probability maps, one float per L0 pixel (arena memory).
  virtual float* run(RunCtx& c, const float* x, Level& L0) = 0;
  // Same from the RGB8 pages themselves (device descriptors, one per image of L0): the normalisation of
  // DetProcessor::preprocess is folded into the first kernel, the f32 input tensor is never built.
  virtual float* run_u8(RunCtx& c, const nn::U8Page* pages, float scale, const float* mean3, const float* std3, Level& L0) = 0;
  virtual const char* arch() const = 0;   // "mobile" / "server"
  virtual const char* dtype() const = 0;  // "f32" / "f16"
  virtual size_t weight_bytes() const = 0;
};
class ClsModel {
 public:
  virtual ~ClsModel() {}
  // x: f32 NHWC pitch-4, n images of 48 x 192. Returns softmax probs [n,2] (arena).
  virtual float* run(RunCtx& c, const float* x, Level& L0) = 0;
  virtual const char* dtype() const = 0;
};
struct SvtrCore;
class RecModel {
 public:
  virtual ~RecModel() {}
  virtual int classes() const = 0;
  int logits_ld() const { return round_up(classes(), 4); }
  // x: f32 NHWC pitch-4 (R,G,B,0), level L0 = lines of height 48; Lt (out) is the token level (H=1, W=T_i).
  // Returns the logits [Lt.total, logits_ld()], or -- with idx_out / prob_out (Lt.total each) -- runs the fused
  // CTC head (argmax + softmax probability of the argmax per time step, no logits in HBM) and returns nullptr.
  // z5_out (rec_return_candidates): receives the head's input features [Lt.total, SvtrCore::D] (arena memory of this pass).
  virtual float* run(RunCtx& c, const float* x, Level& L0, Level& Lt, int* idx_out = nullptr, float* prob_out = nullptr,
                     const float** z5_out = nullptr) = 0;
  virtual const SvtrCore& core() const = 0;   // the head every variant shares (its CTC FC recomputes logits of chosen rows)
  virtual const char* arch() const = 0;
  virtual const char* dtype() const = 0;
  virtual size_t weight_bytes() const = 0;
};

// The part of the recognition head that is the same in every variant (mobile / server, fp32 / fp16): the two
// SVTR mixing blocks + final norm on D = 120 channels, and the CTC FC with its fused argmax epilogue.  fp32.
struct SvtrCore {
  struct Blk { PackedDense qkv, proj, fc1, fc2; float *n1g, *n1b, *n2g, *n2b; } blk[2];
  float *ng = nullptr, *nb = nullptr;
  PackedDense fc;
  int classes = 0, D = 120;
  void load(WeightStore& ws, const Blob& b, const std::string& prefix);  // <prefix>.neck.blk*, .neck.norm, .head.fc
  // z [rows, D] -> LN(blocks(z)) [rows, D]
  float* mixer(RunCtx& c, float* z, const Level& Lt) const;
  // z5 [rows, D] -> fused argmax (idx_out / prob_out) and nullptr, or the logits [rows, round_up(classes, 4)]
  float* head(RunCtx& c, const float* z5, long long rows, int* idx_out, float* prob_out) const;
  // The CTC FC alone over m chosen rows (rec_return_candidates): z_rows [m, D], followed by the zero slack rows every nn::gemm
  // input has, -> out [m, round_up(classes, 4)].  The non-fused GEMM of head(), under a profile family of its own.
  void logits_rows(RunCtx& c, const float* z_rows, long long m, float* out) const;
};

class DetNet : public DetModel {
 public:
  explicit DetNet(const Blob& b);
  float* run(RunCtx& c, const float* x, Level& L0) override { return run(c, x, L0, nullptr, 0.f, nullptr, nullptr); }
  float* run_u8(RunCtx& c, const nn::U8Page* pages, float scale, const float* mean3, const float* std3, Level& L0) override {
    return run(c, nullptr, L0, pages, scale, mean3, std3);
  }
  const char* arch() const override { return "mobile"; }
  const char* dtype() const override { return "f32"; }
  size_t weight_bytes() const override { return ws_.bytes(); }
 private:
  float* run(RunCtx& c, const float* x, Level& L0, const nn::U8Page* pages, float scale, const float* mean3, const float* std3);
  WeightStore ws_;
  float* stem_w_; float* stem_b_;
  std::vector<LcBlock> blocks_;
  int tap_after_[4];
  PackedDense out_[4], ins_[4], inp_[4], head_conv1_;
  float* ins_lin_[4];  // lateral 1x1 weights as [cin][96] for the fused lateral + top-down add
  bool has_bias_[4] = {false, false, false, false};
  SeW ins_se_[4], inp_se_[4];
  float *dc1_w_, *dc1_b_, *dc2_w_, *dc2_b_;
  // nn_fpn.hip operands: head conv split by level (p2 fine / p3 phase / p4, p5 class), inp0 / inp1 phase weights + [tap][n][m] form
  float *head_wf_ = nullptr, *head_wc_ = nullptr, *head_cls4_ = nullptr, *head_cls5_ = nullptr;
  float *inp_wc_[2] = {nullptr, nullptr}, *inp_wm_[2] = {nullptr, nullptr};
};

class RecNet : public RecModel {
 public:
  explicit RecNet(const Blob& b);
  int classes() const override { return core_.classes; }
  float* run(RunCtx& c, const float* x, Level& L0, Level& Lt, int* idx_out = nullptr, float* prob_out = nullptr,
             const float** z5_out = nullptr) override;
  const SvtrCore& core() const override { return core_; }
  const char* arch() const override { return "mobile"; }
  const char* dtype() const override { return "f32"; }
  size_t weight_bytes() const override { return ws_.bytes(); }
  // time steps of a line of width w (stem stride 2, one (1,2) stage, avg-pool 2): the same for the mobile and server graphs
  static int tokens_for_width(int w);
 private:
  WeightStore ws_;
  float* stem_w_; float* stem_b_;
  std::vector<LcBlock> blocks_;
  PackedDense conv1_, conv2_, conv3_, conv4_, conv1x1_;
  SvtrCore core_;
};

class ClsNet : public ClsModel {
 public:
  explicit ClsNet(const Blob& b);
  float* run(RunCtx& c, const float* x, Level& L0) override;
  const char* dtype() const override { return "f32"; }
 private:
  WeightStore ws_;
  float* stem_w_; float* stem_b_;
  std::vector<ClsBlock> blocks_;
  PackedDense conv2_, fc_;
};

}  // namespace rt

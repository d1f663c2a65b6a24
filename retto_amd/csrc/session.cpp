// Session construction (rt_session_create, rt_lane::open / close), the lane's stage-level entries (the networks and the
// pre / post stages on host arrays), the page pipeline (rt_lane::run_pages: one function per stage over the call's Pipeline),
// the results and their stage JSON, and the two debug entries that run a pipeline stage on its own.  How calls reach the lanes
// is session_batch.cpp.
#include "session.h"

#include <charconv>
#include "onnx_import.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <sstream>
#include <chrono>
#include <thread>

#include "geom_math.h"

using namespace rt;

static const bool g_trace = getenv("RT_TRACE") != nullptr;
struct HostTick {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char* what) {
    if (!g_trace) return;
    auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[rt host] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

// ---------------------------------------------------------------------------
// construction (RettoSession::new, session.rs:62-73; RettoWorker::new, worker.rs:91-98)
// ---------------------------------------------------------------------------
rt_session* rt_session_create(const rt_config* cfg) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw RtError(RT_ERR_BACKEND, "no HIP device visible: libretto_hip has no CPU fallback");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) throw RtError(RT_ERR_INVALID, "device_id out of range");
  RT_HIP_CHECK(hipSetDevice(cfg->device_id));
  hipDeviceProp_t prop;
  RT_HIP_CHECK(hipGetDeviceProperties(&prop, cfg->device_id));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    throw RtError(RT_ERR_BACKEND, std::string("libretto_hip is built for gfx950 only, found ") + prop.gcnArchName);
  std::unique_ptr<rt_session> s(new rt_session());
  s->cfg = *cfg;
  s->device = cfg->device_id;
  // model sources are consumed here; do not keep caller pointers
  Blob bd = Blob::from_source(cfg->det.path, cfg->det.data, cfg->det.len, "det", MODEL_DET);
  Blob bc = Blob::from_source(cfg->cls.path, cfg->cls.data, cfg->cls.len, "cls", MODEL_CLS);
  Blob br = Blob::from_source(cfg->rec.path, cfg->rec.data, cfg->rec.len, "rec", MODEL_REC);
  std::vector<uint8_t> dict = read_source_bytes(cfg->dict.path, cfg->dict.data, cfg->dict.len, "dict");
  s->cfg.det = s->cfg.cls = s->cfg.rec = s->cfg.dict = rt_model_source{nullptr, nullptr, 0};
  s->open(s.get());
  // which graph a source holds is read off its tensor names; rt_config.dtype picks the arithmetic
  const bool f16 = cfg->dtype == RT_DTYPE_F16;
  const bool sdet = blob_is_server_det(bd), srec = blob_is_server_rec(br);
  if ((sdet || srec) && !f16)
    throw RtError(RT_ERR_INVALID, "the PP-OCRv4 server graphs are built in fp16 only: set rt_config.dtype = RT_DTYPE_F16");
  if (sdet) s->det.reset(new DetServerH(bd)); else if (f16) s->det.reset(new DetNetH(bd)); else s->det.reset(new DetNet(bd));
  if (f16) s->cls.reset(new ClsNetH(bc)); else s->cls.reset(new ClsNet(bc));
  if (srec) s->rec.reset(new RecServerH(br)); else if (f16) s->rec.reset(new RecNetH(br)); else s->rec.reset(new RecNet(br));
  s->model_info = std::string(s->det->arch()) + "/" + s->det->dtype() + " " + s->cls->dtype() + " " + s->rec->arch() + "/" + s->rec->dtype();
  s->dict = rt::load_dictionary(dict);
  s->charsets.reset(new rt_charsets());
  s->lexicons.reset(new rt_lexicons());
  s->patterns.reset(new rt_patterns());
  s->keywords.reset(new rt_keywords());
  s->lms.reset(new rt_lms());
  s->vocabs.reset(new rt_vocabs());
  if ((int)s->dict.size() != s->rec->classes())
    throw RtError(RT_ERR_SHAPE, "dictionary has " + std::to_string(s->dict.size()) + " entries but the rec head has " +
                                    std::to_string(s->rec->classes()) + " classes");
  if (cfg->rec_return_word_box) {   // the class table of k_word_boxes, once per session
    std::vector<uint8_t> raw(s->dict.size());
    for (size_t i = 0; i < raw.size(); i++) raw[i] = rt::wb::raw_class(s->dict[i].data(), s->dict[i].size());
    RT_HIP_CHECK(hipMalloc((void**)&s->d_word_raw, raw.size()));
    RT_HIP_CHECK(hipMemcpy(s->d_word_raw, raw.data(), raw.size(), hipMemcpyHostToDevice));
  }
  const int lanes = cfg->lanes > 0 ? cfg->lanes : 3;  // measured on C3: 1 -> 640, 2 -> 681, 3 -> 700, 4 -> 652 images/s
  for (int l = 1; l < lanes; l++) {
    s->helpers.emplace_back(new rt_lane());
    s->helpers.back()->open(s.get());
  }
  // CU partitions (RT_LANE_CUMASK=1, A/B only): every lane of a multi-lane session gets its own slice of every XCD.  Measured
  // slower than whole-device streams on C3 (runtime.h "CU partitions"), so the default keeps the lanes time-slicing the chip.
  static const bool part_on = getenv("RT_LANE_CUMASK") && atoi(getenv("RT_LANE_CUMASK")) != 0;
  if (part_on && lanes > 1) {
    std::vector<hipStream_t> ps((size_t)lanes, nullptr);
    std::vector<int> pc((size_t)lanes, 0);
    std::vector<std::vector<unsigned>> ids((size_t)lanes);
    bool ok = true;
    for (int l = 0; l < lanes && ok; l++) ok = (ps[(size_t)l] = rt::partition_stream(l, lanes, &pc[(size_t)l], &ids[(size_t)l])) != nullptr;
    for (int a = 0; a < lanes && ok; a++)
      for (int b = a + 1; b < lanes && ok; b++)
        for (unsigned v : ids[(size_t)a]) if (std::find(ids[(size_t)b].begin(), ids[(size_t)b].end(), v) != ids[(size_t)b].end()) { ok = false; break; }
    if (ok) {
      for (int l = 0; l < lanes; l++) { s->lane(l)->st_part = ps[(size_t)l]; s->lane(l)->part_cus = pc[(size_t)l]; }
    } else {
      for (hipStream_t p : ps) if (p) { rt::forget_stream(p); (void)hipStreamDestroy(p); }
      if (getenv("RT_TRACE")) fprintf(stderr, "[rt] CU partitions could not be verified on this device: lanes keep whole-device streams\n");
    }
  }
  return s.release();
}

void rt_lane::open(const rt_session* session) {
  sh = session;
  RT_HIP_CHECK(hipStreamCreateWithFlags(&st_full, hipStreamNonBlocking));
  st = st_full;
  RT_HIP_CHECK(hipMalloc((void**)&d_flags, 64));
  RT_HIP_CHECK(hipMemset(d_flags, 0, 64));
  RT_HIP_CHECK(hipEventCreateWithFlags(&ev_block, hipEventBlockingSync | hipEventDisableTiming));
}
void rt_lane::close() {
  if (d_flags) (void)hipFree(d_flags);
  if (ev_block) (void)hipEventDestroy(ev_block);
  if (st_part) { rt::forget_stream(st_part); (void)hipStreamDestroy(st_part); }
  if (st_full) (void)hipStreamDestroy(st_full);
  d_flags = nullptr; ev_block = nullptr; st = st_full = st_part = nullptr;
}

void rt_lane::begin_call() {
  RT_HIP_CHECK(hipSetDevice(sh->device));
  (void)hipGetLastError();   // HIP's last error is sticky per host thread: a failure of the PREVIOUS call on this thread (a refused
                             // hipMalloc, say) must not be what the first RT_LAUNCH of this call reports
  if (failed) { arena.abandon_pass(); scratch.abandon_pass(); dbws.abandon_pass(); failed = false; }
  arena.reset(); scratch.reset(); pinned.reset(); dbws.reset();   // (dbws too: its mark below must see the previous pass folded in)
  arena.mark_call(); scratch.mark_call(); dbws.mark_call();
  // (last_error belongs to the API caller's thread -- api_internal.h guarded(); lane threads run this function and never touch it)
}
// Waiting for the lane's stream.  hipStreamSynchronize spins on the CPU (HIP's default scheduling when there are more CPUs than
// GPUs): three lanes = three cores at 100 % per rank for the whole step (measured: 3.9 cores busy per rank), which eight ranks
// on the GPU box's 16-CPU pod do not have.  Here: a blocking-sync event is recorded behind the work, polled for a short while (a
// wait that ends within ~50 us -- single pages, metadata copies -- pays no sleep / wake-up), then polled every 100 us with the
// thread asleep in between.  RT_SYNC_SPIN=1 restores hipStreamSynchronize.
static const bool g_sync_spin = getenv("RT_SYNC_SPIN") && atoi(getenv("RT_SYNC_SPIN")) != 0;
void rt_lane::sync() {
  if (g_sync_spin || !ev_block) {
    RT_HIP_CHECK(hipStreamSynchronize(st));
  } else {
    RT_HIP_CHECK(hipEventRecord(ev_block, st));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t q = hipEventQuery(ev_block);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) RT_HIP_CHECK(q);
      // (hipEventSynchronize on a hipEventBlockingSync event still kept the thread at 100 % of a core on this ROCm: measured
      //  3.0 cores busy with it, 3.9 with hipStreamSynchronize; so the sleeping is done here: poll, sleep 100 us, poll ...)
      //  The spin window is chosen per call: 50 us for multi-page throughput batches, the whole wait (up to 5 ms) for the
      //  single-page / stage-level calls, whose several sync points per call would otherwise pay ~150 us of sleep each.)
      if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
  }
  if (prof.on) prof.collect();
}
void rt_lane::check_flags() {
  int f[2] = {0, 0};
  RT_HIP_CHECK(hipMemcpy(f, d_flags, sizeof(f), hipMemcpyDeviceToHost));
  if (f[0]) {
    RT_HIP_CHECK(hipMemset(d_flags, 0, 64));
    throw RtError(RT_ERR_IMAGE, "thumbnail sampled outside the source image (the reference panics here)");
  }
}

static std::vector<std::pair<int, int>> uniform_hw(int n, int h, int w) {
  return std::vector<std::pair<int, int>>((size_t)n, std::make_pair(h, w));
}

// ---------------------------------------------------------------------------
// L1 worker functions
// ---------------------------------------------------------------------------
// n images of [3, h, w] (host, NCHW) into the arena as the networks read them: NHWC pitch-4
static float* upload_nchw(rt_lane& s, const float* nchw, int n, int h, int w) {
  size_t ne = (size_t)n * 3 * h * w;
  float* d_in = s.arena.alloc<float>(ne);
  RT_HIP_CHECK(hipMemcpyAsync(d_in, nchw, ne * 4, hipMemcpyHostToDevice, s.st));
  float* x = s.arena.alloc<float>((size_t)n * h * w * 4);
  nn::nchw3_to_nhwc4(s.st, d_in, n, h, w, x);
  return x;
}
// ... n lines of [3, h, widths[i]], concatenated (ne floats in all)
static float* upload_ragged(rt_lane& s, const float* nchw, size_t ne, int n, int h, const int* widths) {
  float* d_in = s.arena.alloc<float>(ne);
  RT_HIP_CHECK(hipMemcpyAsync(d_in, nchw, ne * 4, hipMemcpyHostToDevice, s.st));
  float* x = s.arena.alloc<float>(ne / 3 * 4);
  size_t off = 0;
  for (int i = 0; i < n; i++) {
    nn::nchw3_to_nhwc4(s.st, d_in + off * 3, 1, h, widths[i], x + off * 4);
    off += (size_t)h * widths[i];
  }
  return x;
}
void rt_lane::det_forward(const float* nchw, int n, int h, int w, float* out) {
  begin_call();
  float* x = upload_nchw(*this, nchw, n, h, w);
  Level L0 = make_level(uniform_hw(n, h, w));
  RunCtx c = ctx(&scratch);
  float* map = sh->det->run(c, x, L0);
  RT_HIP_CHECK(hipMemcpyAsync(out, map, (size_t)n * h * w * 4, hipMemcpyDeviceToHost, st));
  sync();
}
void rt_lane::cls_forward(const float* nchw, int n, int h, int w, float* out) {
  begin_call();
  float* x = upload_nchw(*this, nchw, n, h, w);
  Level L0 = make_level(uniform_hw(n, h, w));
  RunCtx c = ctx(&scratch);
  float* probs = sh->cls->run(c, x, L0);
  RT_HIP_CHECK(hipMemcpyAsync(out, probs, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, st));
  sync();
}
void rt_lane::rec_forward(const float* nchw, int n, int h, int w, float* out, int* t_out) {
  int T = RecNet::tokens_for_width(w);
  if (t_out) *t_out = T;
  if (!out) return;
  begin_call();
  float* x = upload_nchw(*this, nchw, n, h, w);
  Level L0 = make_level(uniform_hw(n, h, w)), Lt;
  RunCtx c = ctx(&scratch);
  float* logits = sh->rec->run(c, x, L0, Lt);
  const int C = sh->rec->classes();
  float* probs = scratch.alloc<float>((size_t)Lt.total * C);
  nn::softmax_rows(st, logits, sh->rec->logits_ld(), Lt.total, C, probs);
  RT_HIP_CHECK(hipMemcpyAsync(out, probs, (size_t)Lt.total * C * 4, hipMemcpyDeviceToHost, st));
  sync();
}

// Ragged form of rec_forward: line i is [3,48,widths[i]] (NCHW, lines concatenated), every line keeps its own width inside ONE
// launch series -- what rt_run_batch's rec groups do (rec_processor.rs:214-270 gives each batch of 6 its width; the session
// concatenates the batches).  out = the lines' [T_i, classes] probabilities concatenated, t_out[i] = T_i.
void rt_lane::rec_forward_ragged(const float* nchw, int n, const int* widths, float* out, int* t_out) {
  const int h = 48;
  size_t ne = 0, nt = 0;
  for (int i = 0; i < n; i++) {
    if (widths[i] < 8) throw RtError(RT_ERR_SHAPE, "rt_rec_ragged: every line must be at least 8 wide");
    ne += (size_t)3 * h * widths[i];
    int T = RecNet::tokens_for_width(widths[i]);
    if (t_out) t_out[i] = T;
    nt += (size_t)T;
  }
  if (!out) return;
  begin_call();
  float* x = upload_ragged(*this, nchw, ne, n, h, widths);
  std::vector<std::pair<int, int>> hw;
  for (int i = 0; i < n; i++) hw.emplace_back(h, widths[i]);
  Level L0 = make_level(hw), Lt;
  RunCtx c = ctx(&scratch);
  float* logits = sh->rec->run(c, x, L0, Lt);
  if ((size_t)Lt.total != nt) throw RtError(RT_ERR_BACKEND, "rt_rec_ragged: token count mismatch");
  const int C = sh->rec->classes();
  float* probs = scratch.alloc<float>((size_t)Lt.total * C);
  nn::softmax_rows(st, logits, sh->rec->logits_ld(), Lt.total, C, probs);
  RT_HIP_CHECK(hipMemcpyAsync(out, probs, (size_t)Lt.total * C * 4, hipMemcpyDeviceToHost, st));
  sync();
}

// ---------------------------------------------------------------------------
// stage functions
// ---------------------------------------------------------------------------
// image_helper.rs:106-148 on a device image; returns the (possibly new) device buffer
static const uint8_t* dev_resize_both(rt_lane* s, const uint8_t* img, int h, int w, int* oh, int* ow) {
  int plan[4];
  int n = gm::resize_both_plan(h, w, s->sh->cfg.max_side_len, s->sh->cfg.min_side_len, plan);
  const uint8_t* cur = img; int ch = h, cw = w;
  for (int i = 0; i < n; i++) {
    int nh = plan[2 * i], nw = plan[2 * i + 1];
    uint8_t* dst = s->arena.alloc<uint8_t>(std::max<size_t>((size_t)nh * nw * 3, 4));
    ProfScope ps(&s->prof, s->st, "thumbnail");
    pp::thumbnail_rgb8(s->st, cur, ch, cw, dst, nh, nw, s->d_flags);
    cur = dst; ch = nh; cw = nw;
  }
  *oh = ch; *ow = cw;
  return cur;
}

void rt_lane::resize_both(const uint8_t* rgb, int h, int w, uint8_t* out, int oh, int ow) {
  begin_call();
  uint8_t* d = arena.alloc<uint8_t>((size_t)h * w * 3);
  RT_HIP_CHECK(hipMemcpyAsync(d, rgb, (size_t)h * w * 3, hipMemcpyHostToDevice, st));
  int rh, rw;
  const uint8_t* r = dev_resize_both(this, d, h, w, &rh, &rw);
  if (rh != oh || rw != ow) throw RtError(RT_ERR_SHAPE, "resize_both: output buffer dims do not match rt_resize_both_dims");
  RT_HIP_CHECK(hipMemcpyAsync(out, r, (size_t)rh * rw * 3, hipMemcpyDeviceToHost, st));
  sync(); check_flags();
}

void rt_lane::det_preprocess(const uint8_t* rgb, int h, int w, float* out) {
  begin_call();
  uint8_t* d = arena.alloc<uint8_t>((size_t)h * w * 3);
  RT_HIP_CHECK(hipMemcpyAsync(d, rgb, (size_t)h * w * 3, hipMemcpyHostToDevice, st));
  int dh, dw;
  gm::resize_either_dims(h, w, sh->cfg.det_limit_type, sh->cfg.det_limit_side_len, &dh, &dw);
  if (dh <= 0 || dw <= 0) throw RtError(RT_ERR_SHAPE, "det input collapses to zero size");
  uint8_t* r = arena.alloc<uint8_t>((size_t)dh * dw * 3);
  pp::thumbnail_rgb8(st, d, h, w, r, dh, dw, d_flags);
  float* o = arena.alloc<float>((size_t)dh * dw * 3);
  pp::det_normalize(st, r, dh, dw, sh->cfg.det_scale, sh->cfg.det_mean, sh->cfg.det_std, 1, o);
  RT_HIP_CHECK(hipMemcpyAsync(out, o, (size_t)dh * dw * 3 * 4, hipMemcpyDeviceToHost, st));
  sync(); check_flags();
}

static pp::DbParams db_params(const rt_config& c) {
  pp::DbParams p;
  p.thresh = c.det_thresh; p.box_thresh = c.det_box_thresh; p.unclip_ratio = c.det_unclip_ratio;
  p.min_size = c.det_min_mini_box_size; p.dilate = c.det_dilation;
  p.score_mode = c.det_score_mode;
  return p;
}
static int max_boxes_of(const rt_config& c) { return c.max_boxes_per_page > 0 ? c.max_boxes_per_page : 8192; }

// a5 (det_processor.rs:279-335) enqueued for n pages with shared launches: page i's boxes go to boxes[i * max_boxes_of ...],
// its count and overflow flag to counts[2 i], counts[2 i + 1]
static void db_post_enqueue(rt_lane& s, int n, const pp::DbPageIn* in, pp::DbBox* boxes, int* counts) {
  const int mb = max_boxes_of(s.sh->cfg);
  std::vector<void*> wsp((size_t)n); std::vector<pp::DbBox*> bo((size_t)n); std::vector<int*> co((size_t)n);
  for (int i = 0; i < n; i++) {
    wsp[i] = s.dbws.alloc_bytes(pp::db_workspace_bytes(in[i].H, in[i].W, mb, s.sh->cfg.det_score_mode));
    bo[i] = boxes + (size_t)i * mb; co[i] = counts + 2 * i;
  }
  void* hd = s.pinned.alloc_bytes((size_t)n * pp::db_page_desc_bytes());
  void* dd = s.arena.alloc_bytes((size_t)n * pp::db_page_desc_bytes());
  pp::db_postprocess_batch(s.st, n, in, db_params(s.sh->cfg), wsp.data(), mb, bo.data(), co.data(), hd, dd);
}

void rt_lane::det_postprocess(const float* pred, int h, int w, int ori_h, int ori_w, float* boxes, float* scores,
                                 int max_out, int* n_out) {
  begin_call();
  float* d = arena.alloc<float>((size_t)h * w);
  RT_HIP_CHECK(hipMemcpyAsync(d, pred, (size_t)h * w * 4, hipMemcpyHostToDevice, st));
  pp::DbBox* db = arena.alloc<pp::DbBox>(max_boxes_of(sh->cfg));
  int* cnt = arena.alloc<int>(2);
  const pp::DbPageIn in{d, h, w, ori_h, ori_w};
  db_post_enqueue(*this, 1, &in, db, cnt);
  int hc[2];
  RT_HIP_CHECK(hipMemcpyAsync(hc, cnt, 8, hipMemcpyDeviceToHost, st));
  sync();
  if (hc[1]) throw RtError(RT_ERR_CAPACITY, "DB post-processing work list overflow (raise max_boxes_per_page)");
  *n_out = hc[0];
  int n = std::min(hc[0], max_out);
  std::vector<pp::DbBox> hb((size_t)std::max(n, 1));
  if (n > 0) RT_HIP_CHECK(hipMemcpy(hb.data(), db, (size_t)n * sizeof(pp::DbBox), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) { memcpy(boxes + 8 * i, hb[i].pts, 32); scores[i] = hb[i].score; }
}

struct CropPlan {
  std::vector<pp::CropDesc> descs;
  std::vector<pp::CropRef> refs;
  std::vector<gm::CropDims> dims;   // per crop: what the word boxes map back through (cw, ch)
  size_t pool_bytes = 0;
  int max_pix = 0;
  long long total_pix = 0;          // sum of w * h: the flat warp's work list (CropDesc::pix_base is its prefix sum)
};
// image_helper.rs:223-249 planning for one box b[8] of a page (src = the device page the crop is cut from: the page after
// resize_both, or the caller's page with crop_source = Original and in rt_run_regions; b in that page's coordinates)
static void plan_crop(CropPlan& plan, const uint8_t* src, int sh, int sw, const float* b) {
  gm::CropDims d = gm::crop_dims(b);
  if (d.w <= 0 || d.h <= 0) throw RtError(RT_ERR_IMAGE, "zero-sized crop");
  if ((long long)d.w * d.h > 0x7fffffffLL) throw RtError(RT_ERR_IMAGE, "crop of more than 2^31 pixels");
  pp::CropDesc cd;
  cd.src = src; cd.sh = sh; cd.sw = sw; cd.w = d.w; cd.h = d.h; cd.rot = d.rot;
  if (!gm::projection_inverse(b, d.cw, d.ch, cd.inv))
    throw RtError(RT_ERR_IMAGE, "singular crop homography (Projection::from_control_points -> None; the reference unwraps)");
  cd.out_off = (long long)plan.pool_bytes;
  cd.pix_base = plan.total_pix;
  pp::CropRef r; r.off = cd.out_off; r.h = d.rot ? d.w : d.h; r.w = d.rot ? d.h : d.w; r.pad_ = 0;
  plan.descs.push_back(cd); plan.refs.push_back(r); plan.dims.push_back(d);
  plan.pool_bytes += ((size_t)d.w * d.h * 3 + 63) & ~(size_t)63;
  plan.max_pix = std::max(plan.max_pix, d.w * d.h);
  plan.total_pix += (long long)d.w * d.h;
}
// a6: the plan's descriptors and crop refs to the device through pinned staging, then every crop warped into one pool (returned;
// *d_refs: the refs on the device, what cls_post_rotate reads).  The plan holds at least one crop.  flat: the launch walks the
// flat pixel list (crops of very different sizes: original-page crops, caller-supplied regions) instead of one grid row per crop.
static uint8_t* warp_planned_crops(rt_lane& s, const CropPlan& plan, pp::CropRef** d_refs, bool flat) {
  const int n = (int)plan.descs.size();
  uint8_t* pool = s.arena.alloc<uint8_t>(plan.pool_bytes + 64);
  pp::CropDesc* d_desc = s.arena.alloc<pp::CropDesc>(n);
  *d_refs = s.arena.alloc<pp::CropRef>(n);
  pp::CropDesc* hd = s.pinned.alloc<pp::CropDesc>(n);
  pp::CropRef* hr = s.pinned.alloc<pp::CropRef>(n);
  memcpy(hd, plan.descs.data(), (size_t)n * sizeof(pp::CropDesc));
  memcpy(hr, plan.refs.data(), (size_t)n * sizeof(pp::CropRef));
  RT_HIP_CHECK(hipMemcpyAsync(d_desc, hd, (size_t)n * sizeof(pp::CropDesc), hipMemcpyHostToDevice, s.st));
  RT_HIP_CHECK(hipMemcpyAsync(*d_refs, hr, (size_t)n * sizeof(pp::CropRef), hipMemcpyHostToDevice, s.st));
  ProfScope ps(&s.prof, s.st, "warp_crops");
  if (flat) pp::warp_crops_flat(s.st, d_desc, n, plan.total_pix, pool);
  else pp::warp_crops(s.st, d_desc, n, plan.max_pix, pool);
  return pool;
}

void rt_lane::crop_images(const uint8_t* rgb, int h, int w, const float* boxes, int n, uint8_t* out, size_t out_cap, int form) {
  begin_call();
  uint8_t* d = arena.alloc<uint8_t>((size_t)h * w * 3);
  RT_HIP_CHECK(hipMemcpyAsync(d, rgb, (size_t)h * w * 3, hipMemcpyHostToDevice, st));
  CropPlan plan;
  for (int i = 0; i < n; i++) plan_crop(plan, d, h, w, boxes + 8 * i);
  size_t need = 0;
  for (auto& r : plan.refs) need += (size_t)r.h * r.w * 3;
  if (need > out_cap) throw RtError(RT_ERR_INVALID, "crop_images: output buffer too small");
  if (n > 0) {
    pp::CropRef* d_refs;
    const uint8_t* pool = warp_planned_crops(*this, plan, &d_refs, form == 1);
    for (const pp::CropRef& r : plan.refs) {
      const size_t bytes = (size_t)r.h * r.w * 3;
      RT_HIP_CHECK(hipMemcpyAsync(out, pool + r.off, bytes, hipMemcpyDeviceToHost, st));
      out += bytes;
    }
  }
  sync();
}

// image_helper.rs:176-209: the line of crop r resized to height img_h and padded to width W; the resized width follows the
// crop's original dims ori_h x ori_w (inside the pipeline: the crop's own dims)
static pp::LineDesc line_desc(const pp::CropRef& r, int ori_h, int ori_w, int img_h, int W) {
  return pp::LineDesc{r.off, r.h, r.w, gm::resize_norm_resized_w(img_h, W, ori_h, ori_w), W, 0};
}

void rt_lane::resize_norm_image(const uint8_t* crop, int h, int w, int ori_h, int ori_w, int img_h, int img_w,
                                   float ratio, float* out) {
  begin_call();
  uint8_t* d = arena.alloc<uint8_t>(std::max<size_t>((size_t)h * w * 3, 4));
  RT_HIP_CHECK(hipMemcpyAsync(d, crop, (size_t)h * w * 3, hipMemcpyHostToDevice, st));
  pp::LineDesc* hl = pinned.alloc<pp::LineDesc>(1);
  const int W = gm::resize_norm_width(img_h, img_w, ratio);
  *hl = line_desc(pp::CropRef{0, h, w, 0}, ori_h, ori_w, img_h, W);
  pp::LineDesc* dl = arena.alloc<pp::LineDesc>(1);
  RT_HIP_CHECK(hipMemcpyAsync(dl, hl, sizeof(pp::LineDesc), hipMemcpyHostToDevice, st));
  float* o = arena.alloc<float>((size_t)3 * img_h * std::max(W, 1));
  pp::resize_norm(st, dl, 1, img_h, W, d, 1, o, d_flags);
  RT_HIP_CHECK(hipMemcpyAsync(out, o, (size_t)3 * img_h * W * 4, hipMemcpyDeviceToHost, st));
  sync(); check_flags();
}

void rt_lane::ctc_decode(const float* probs, int n, int t, int c, int32_t* idx, float* prob, int32_t* tokens,
                            int32_t* n_tokens, float* scores) {
  begin_call();
  size_t rows = (size_t)n * t;
  float* d = arena.alloc<float>(rows * c);
  RT_HIP_CHECK(hipMemcpyAsync(d, probs, rows * c * 4, hipMemcpyHostToDevice, st));
  int* di = arena.alloc<int>(rows); float* dp = arena.alloc<float>(rows);
  int* dt = arena.alloc<int>(rows); int* dn = arena.alloc<int>(n); float* ds = arena.alloc<float>(n);
  // per (n,t): first argmax and max of the probabilities themselves (rec_processor.rs:198-199)
  Level Lt = make_level(uniform_hw(n, 1, t));
  RunCtx cx = ctx(&arena);
  upload_levels(cx, {&Lt});
  nn::argmax_rows(st, d, c, (long long)rows, c, di, dp);
  pp::ctc_decode(st, di, dp, Lt.d, n, dt, dn, ds);
  RT_HIP_CHECK(hipMemcpyAsync(idx, di, rows * 4, hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(hipMemcpyAsync(prob, dp, rows * 4, hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(hipMemcpyAsync(tokens, dt, rows * 4, hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(hipMemcpyAsync(n_tokens, dn, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(hipMemcpyAsync(scores, ds, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  sync();
}

namespace {
std::string json_escape(const std::string& s) {
  std::string o;
  for (char ch : s) {
    switch (ch) {
      case '"': o += "\\\""; break;
      case '\\': o += "\\\\"; break;
      case '\n': o += "\\n"; break;
      case '\r': o += "\\r"; break;
      case '\t': o += "\\t"; break;
      default:
        if ((unsigned char)ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", ch); o += b; }
        else o += ch;
    }
  }
  return o;
}
// serde_json writes a finite f32 through ryu: the shortest decimal string that parses back to the same f32
// (0.9f -> "0.9", not "0.899999976"), laid out by ryu's f32 rules -- plain decimals while the decimal point
// position kk is in (-6, 13] ("123.0", "0.00001234"), otherwise d[.ddd]e[-]x ("1e30", "1.234e-7").
std::string fnum(float v) {
  if (v != v || std::isinf(v)) return "null";  // serde_json writes non-finite floats as null
  if (v == 0.0f) return std::signbit(v) ? "-0.0" : "0.0";
  // std::to_chars (scientific, no precision) yields exactly the shortest digit string that round-trips, and -- unlike
  // snprintf / strtof -- does not depend on LC_NUMERIC (a host that called setlocale() with a comma-decimal locale would
  // otherwise get invalid JSON)
  char b[48];
  const std::to_chars_result tr = std::to_chars(b, b + sizeof b - 1, v, std::chars_format::scientific);
  *tr.ptr = 0;
  std::string digits; int exp10 = 0; bool neg = false;
  {
    const char* p = b;
    if (*p == '-') { neg = true; p++; }
    for (; *p && *p != 'e'; p++) if (*p != '.') digits += *p;
    exp10 = atoi(p + 1);
  }
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  const int len = (int)digits.size();
  const int k = exp10 - (len - 1);  // value = digits * 10^k
  const int kk = len + k;           // position of the decimal point
  std::string o = neg ? "-" : "";
  if (0 <= k && kk <= 13) { o += digits; o.append((size_t)k, '0'); o += ".0"; }
  else if (0 < kk && kk <= 13) { o += digits.substr(0, (size_t)kk); o += '.'; o += digits.substr((size_t)kk); }
  else if (-6 < kk && kk <= 0) { o += "0."; o.append((size_t)(-kk), '0'); o += digits; }
  else {
    o += digits[0];
    if (len > 1) { o += '.'; o += digits.substr(1); }
    o += 'e'; o += std::to_string(kk - 1);
  }
  return o;
}

// RettoWorkerStageResult JSON (serde derive shapes; retto-wasm/fe/index.ts:5-42)
std::string stage_json(const rt_results::Page& P, int stage) {
  std::ostringstream o;
  size_t n = P.det_scores.size();
  if (stage == 0) {
    o << "[";
    for (size_t k = 0; k < n; k++) {
      if (k) o << ",";
      o << "{\"boxes\":{\"inner\":[";
      for (int q = 0; q < 4; q++) { if (q) o << ","; o << "{\"x\":" << fnum(P.boxes[8 * k + 2 * q]) << ",\"y\":" << fnum(P.boxes[8 * k + 2 * q + 1]) << "}"; }
      o << "]},\"score\":" << fnum(P.det_scores[k]) << "}";
    }
    o << "]";
  } else if (stage == 1) {
    o << "[";
    for (size_t k = 0; k < n; k++) { if (k) o << ","; o << "{\"label\":{\"label\":" << P.cls_labels[k] << ",\"score\":" << fnum(P.cls_scores[k]) << "}}"; }
    o << "]";
  } else {
    o << "[";
    for (size_t k = 0; k < n; k++) { if (k) o << ","; o << "{\"text\":\"" << json_escape(P.text[k]) << "\",\"score\":" << fnum(P.rec_scores[k]) << "}"; }
    o << "]";
  }
  return o.str();
}
// run_stream: page `page` of the call has completed `stage` -- its JSON to the call's callback, under the call's mutex
void emit_stage(const PageCall& call, int page, int stage, const rt_results::Page& P) {
  if (!call.cb) return;
  const std::string j = stage_json(P, stage);
  std::unique_lock<std::mutex> lk;
  if (call.cb_mu) lk = std::unique_lock<std::mutex>(*call.cb_mu);
  call.cb(call.user, call.page_base + page, stage, j.c_str());
}

// ---------------------------------------------------------------------------
// L2: process_pipeline over a batch of pages, one function per stage over the call's state
// ---------------------------------------------------------------------------
struct PageState {
  int ori_h, ori_w, after_h, after_w, det_h, det_w;
  const uint8_t* raw;      // device, the caller's page (ori_h x ori_w): what crop_source = Original and the regions are cut from
  const uint8_t* img;      // device, after resize_both
  const uint8_t* det_img;  // device, det input size (RGB8: the det stem normalises it)
  const float* map;        // device det map used for boxes
  int n_boxes = 0; int first_line = 0;
  const pp::DbBox* boxes = nullptr;  // pinned: the page's part of round trip #1 (regions: the caller's clamped quads, host)
};
// per-line results: views of one [4][NLp] block of 32-bit words (label first), so that one copy brings them to the host
struct LineMeta {
  int* label = nullptr; float* cscore = nullptr; int* ntok = nullptr; float* rscore = nullptr;
  void view(int* m, int NLp) { label = m; cscore = reinterpret_cast<float*>(m + NLp); ntok = m + 2 * NLp; rscore = reinterpret_cast<float*>(m + 3 * NLp); }
};
// A per-call result array that the tail fills per line: [n] on the device (from `arena`) with its mirror in pinned memory, both
// allocated at once so that one count sizes them; fetch() queues the copy home.  Null until allocated: the option is off.
template <typename T>
struct Mirror {
  T* d = nullptr; T* h = nullptr; size_t n = 0;
  void alloc(rt_lane& s, size_t n_) { n = n_; d = s.arena.alloc<T>(n); h = s.pinned.alloc<T>(n); }
  void fetch(hipStream_t st) const { if (d) RT_HIP_CHECK(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, st)); }
};
// the state of one run_pages call; device and pinned buffers live until the next begin_call
struct Pipeline {
  const PageCall& call;
  std::vector<PageState> pg;
  std::vector<pp::DbBox> region_boxes;            // rt_run_regions: the caller's boxes as the stages read them (score 1)
  bool crop_original = false;                     // crops are planned on PageState::raw (regions, or crop_source = Original)
  std::vector<double*> sum_parts; std::vector<int> sum_counts;   // det map checksum partials per det group or page map (device)
  float* tile_maps_out = nullptr;           // rt_debug_det_tiles: host, every tile's own map packed in plan order (one-page call)
  int* d_counts = nullptr;                  // [n_pages][2]: box count, overflow flag
  pp::DbBox* d_boxes_packed = nullptr;      // every page's boxes, packed in page order
  int NL = 0, NLp = 1;                      // lines of the call; NLp = max(NL, 1) sizes the per-line buffers
  CropPlan plan; uint8_t* pool = nullptr; pp::CropRef* d_refs = nullptr;   // the crops: their plan, pool and refs (device)
  LineMeta h_meta, d_meta;
  std::vector<pp::LineDesc> lines; std::vector<int> line_W;  // rec: per line its resize_norm descriptor and width
  std::vector<long long> tok_off;           // [NL + 1]: first token of every line
  int* d_tok = nullptr; int* h_tokens = nullptr;   // CTC tokens at tok_off
  int* d_wcount = nullptr; wb::Word* d_words = nullptr; int* h_wcount = nullptr; wb::Word* h_words = nullptr;   // rec_return_word_box
  int* d_ccol = nullptr; cc::Cand* d_cands = nullptr; int* h_ccol = nullptr; cc::Cand* h_cands = nullptr;       // rec_return_candidates
  // per line its charset, lexicon and pattern (0: none), and per kind whether some line of the call has one (rec_line_opts.h)
  std::vector<RecLineOpts> line_opts; RecLineAny any;
  // rec lexicons (any.lexicon): per line lx::MATCHES match slots and the number of matches (written for the lines that carry a
  // lexicon only)
  Mirror<lx::Match> lexm; Mirror<int> lexn;
  // lexicon snap (ctc_lexicon_align.h): per line 1 where it snapped; null unless a lexicon of the call's lines has snap on
  Mirror<int> lexs;
  // rec patterns (ctc_pattern.h; any.pattern): per line matched | vit | logprob | free_logprob, one block of 4 NLp words (written
  // for the lines that carry a pattern only)
  Mirror<int> pat;
  // rec keywords (ctc_keyword.h; any.keywords): per line kw::HITS hit slots and the number of hits (written for the lines that
  // carry a list only)
  Mirror<kw::Hit> kwh; Mirror<int> kwn;
  // rec beams (ctc_beam.h; call.set.beam_b > 0).  Per line its count and beam_n records; the token pool: line li's hypothesis k
  // at [(tok_off[li] * beam_n) + k * T]
  Mirror<int> bmn; Mirror<bm::Beam> bmrec; Mirror<int> bmtok;
  // rec language model (ctc_lm.h; call.set.fused()): per record slot lm and the fused score; null otherwise
  Mirror<lm::BeamLm> bmlm;
  // rec vocabulary (ctc_vocab.h; call.set.worded()): per record slot the closed count and the closing score; null otherwise
  Mirror<vc::BeamVocab> bmvc;
  // rec flip (rec_flip.h; call.set.flip_cls_below > 0): per line whether it is read both ways (host; empty: no line of the call
  // is), and then per line its outcome (zeroed: 0 = read one way) and the two views' scores
  std::vector<uint8_t> both; Mirror<int> flipo; Mirror<float> flips;
};

// Launch groups: items [g0, end) where the group always takes its first item; with max_items > 0 it takes up to max_items items,
// otherwise items while their pixels px_of(i) sum to at most budget_px.
template <class PxOf>
int group_end(int g0, int n, int max_items, long long budget_px, PxOf px_of) {
  int g1 = g0; long long px = 0;
  while (g1 < n) {
    const long long add = px_of(g1);
    if (g1 > g0 && (max_items > 0 ? g1 - g0 >= max_items : px + add > budget_px)) break;
    px += add; g1++;
  }
  return g1;
}
// a page's boxes (after_* coordinates) to original-image corners, and their scores (session.rs:94-105)
// (regions: the quads are reported as they were clamped, unrounded)
void page_boxes(const PageState& p, rt_results::Page& P, bool regions) {
  P.boxes.resize((size_t)p.n_boxes * 8); P.det_scores.resize((size_t)p.n_boxes);
  for (int k = 0; k < p.n_boxes; k++) {
    memcpy(&P.boxes[8 * k], p.boxes[k].pts, 32);
    if (!regions) gm::scale_and_clip(&P.boxes[8 * k], (double)p.after_w, (double)p.after_h, (double)p.ori_w, (double)p.ori_h);
    P.det_scores[k] = p.boxes[k].score;
  }
}
// page i of the call in HBM: the caller's device pointer, or an upload
const uint8_t* page_on_device(rt_lane& s, const PageCall& c, int i) {
  const uint8_t* const* rgb = c.rgb; const int* hs = c.hs; const int* ws = c.ws;
  if (hs[i] <= 0 || ws[i] <= 0 || rgb[i] == nullptr) throw RtError(RT_ERR_IMAGE, "empty page");
  if (c.mem != RT_MEM_HOST && c.mem != RT_MEM_HOST_MAPS_DEVICE) return rgb[i];
  // the pages cross PCIe here (a submitted batch staged them already)
  uint8_t* d = s.arena.alloc<uint8_t>((size_t)hs[i] * ws[i] * 3);
  RT_HIP_CHECK(hipMemcpyAsync(d, rgb[i], (size_t)hs[i] * ws[i] * 3, hipMemcpyHostToDevice, s.st));
  return d;
}
// ---- a2 + a3: size limits, det resize (the normalise is folded into the det stem) ----
void page_sizes(rt_lane& s, Pipeline& P) {
  const int* hs = P.call.hs; const int* ws = P.call.ws;
  // a det input beyond what DB post-processing indexes (det_tiles.h "The largest det input") is refused before anything is queued
  for (int i = 0; i < P.call.n_pages; i++) {
    if (hs[i] <= 0 || ws[i] <= 0) continue;   // (an empty page: page_on_device reports it)
    int plan[4], ah = hs[i], aw = ws[i], dh = 0, dw = 0;
    const int n = gm::resize_both_plan(hs[i], ws[i], s.sh->cfg.max_side_len, s.sh->cfg.min_side_len, plan);
    if (n > 0) { ah = plan[2 * (n - 1)]; aw = plan[2 * (n - 1) + 1]; }
    if (ah <= 0 || aw <= 0) continue;
    gm::resize_either_dims(ah, aw, s.sh->cfg.det_limit_type, s.sh->cfg.det_limit_side_len, &dh, &dw);
    std::string why;
    if (dh > 0 && dw > 0 && dt::check_page(dh, dw, &why) == dt::ERR_CAPACITY) throw RtError(RT_ERR_CAPACITY, "page " + std::to_string(i) + ": " + why);
  }
  for (int i = 0; i < P.call.n_pages; i++) {
    PageState& p = P.pg[i];
    p.ori_h = hs[i]; p.ori_w = ws[i];
    const uint8_t* raw = p.raw = page_on_device(s, P.call, i);
    p.img = dev_resize_both(&s, raw, hs[i], ws[i], &p.after_h, &p.after_w);
    if (p.after_h <= 0 || p.after_w <= 0) throw RtError(RT_ERR_SHAPE, "page collapses to zero size in resize_both");
    gm::resize_either_dims(p.after_h, p.after_w, s.sh->cfg.det_limit_type, s.sh->cfg.det_limit_side_len, &p.det_h, &p.det_w);
    if (p.det_h <= 0 || p.det_w <= 0) throw RtError(RT_ERR_SHAPE, "det input collapses to zero size");
    if (p.det_h == p.after_h && p.det_w == p.after_w) p.det_img = p.img;  // thumbnail at ratio 1 is the identity
    else {
      uint8_t* d = s.arena.alloc<uint8_t>((size_t)p.det_h * p.det_w * 3);
      ProfScope ps(&s.prof, s.st, "thumbnail");
      pp::thumbnail_rgb8(s.st, p.img, p.after_h, p.after_w, d, p.det_h, p.det_w, s.d_flags);
      p.det_img = d;
    }
  }
}
// ---- a4: det network in launch groups ----------------------------------------------
// The items of the launch groups are UNITS: an untiled page, or one tile of a tiled page (det tiles, det_tiles.h: a page whose det
// input is larger than the call's tile either way).  The units of all pages are mixed under the one pixel budget and the one
// det_sub_batch rule.  A tiled page's map is an arena allocation of det_h * det_w floats; a group's tiles are cut out of their
// pages (k_det_tile_cut) into the contiguous RGB8 form run_u8 reads, and after the group's network run their owned rectangles are
// written into the page maps (k_det_tile_stitch), before the next group rewinds the scratch arena.  Without a tiled page in the
// call every group is what it was before tiles existed: the same launches, the same bits.
struct DetUnit { int page, ty, tx, h, w; };   // ty < 0: the whole page
void det_groups(rt_lane& s, Pipeline& P) {
  const long long group_px = (long long)32 * 960 * 960;  // measured: larger launch groups win (launch-bound small layers)
  const int T = P.call.set.det_tile, O = P.call.set.det_overlap;
  std::vector<DetUnit> units;
  std::vector<dt::Axis> rows((size_t)P.call.n_pages), cols((size_t)P.call.n_pages);
  std::vector<float*> page_map((size_t)P.call.n_pages, nullptr);
  for (int i = 0; i < P.call.n_pages; i++) {
    const PageState& p = P.pg[i];
    if (!dt::page_tiled(p.det_h, p.det_w, T)) { units.push_back(DetUnit{i, -1, -1, p.det_h, p.det_w}); continue; }
    rows[(size_t)i] = dt::axis_plan(p.det_h, T, O); cols[(size_t)i] = dt::axis_plan(p.det_w, T, O);
    P.pg[i].map = page_map[(size_t)i] = s.arena.alloc<float>((size_t)p.det_h * p.det_w);
    for (int ty = 0; ty < rows[(size_t)i].n(); ty++)
      for (int tx = 0; tx < cols[(size_t)i].n(); tx++) units.push_back(DetUnit{i, ty, tx, rows[(size_t)i].len, cols[(size_t)i].len});
  }
  // a map's checksum partials (device): they ride home with the box counts
  const auto checksum = [&](const float* m, long long px) {
    const int nb = pp::sum_blocks(px);
    double* parts = s.arena.alloc<double>(nb);
    pp::sum_partial(s.st, m, px, parts);
    P.sum_parts.push_back(parts); P.sum_counts.push_back(nb);
  };
  const int nu = (int)units.size();
  for (int g0 = 0; g0 < nu;) {
    const int g1 = group_end(g0, nu, s.sh->cfg.det_sub_batch, group_px, [&](int i) { return (long long)units[(size_t)i].h * units[(size_t)i].w; });
    const int gn = g1 - g0;
    std::vector<std::pair<int, int>> hw;
    int nt = 0;
    for (int i = g0; i < g1; i++) { hw.push_back({units[(size_t)i].h, units[(size_t)i].w}); nt += units[(size_t)i].ty >= 0; }
    Level L0 = make_level(hw);
    s.scratch.rewind();
    // the pages stay RGB8 until the first conv reads them (DetNet::run_u8)
    nn::U8Page* hd = s.pinned.alloc<nn::U8Page>((size_t)gn);
    nn::U8Page* dd = s.scratch.alloc<nn::U8Page>((size_t)gn);
    // the group's tiles: their descriptors through pinned into scratch, as the crop refs go, and the buffer they are cut into
    dt::TileDesc* ht = nullptr; dt::TileDesc* d_tiles = nullptr;
    long long max_tile_pix = 0;
    if (nt > 0) {
      ht = s.pinned.alloc<dt::TileDesc>((size_t)nt);
      d_tiles = s.scratch.alloc<dt::TileDesc>((size_t)nt);
      size_t cut_bytes = 0;
      int k = 0;
      for (int i = g0; i < g1; i++) {
        const DetUnit& u = units[(size_t)i];
        if (u.ty < 0) continue;
        const dt::Axis& R = rows[(size_t)u.page]; const dt::Axis& C = cols[(size_t)u.page];
        dt::TileDesc& t = ht[k++];
        t.src = P.pg[u.page].det_img; t.page_map = page_map[(size_t)u.page]; t.page_w = P.pg[u.page].det_w;
        t.cut_off = (long long)cut_bytes; t.map_off = L0.h[i - g0].off;
        t.y0 = R.origin[(size_t)u.ty]; t.x0 = C.origin[(size_t)u.tx]; t.th = u.h; t.tw = u.w;
        t.oy0 = R.own0(u.ty); t.oy1 = R.bound[(size_t)u.ty]; t.ox0 = C.own0(u.tx); t.ox1 = C.bound[(size_t)u.tx]; t.pad_ = 0;
        cut_bytes += ((size_t)u.h * u.w * 3 + 255) & ~(size_t)255;
        max_tile_pix = std::max(max_tile_pix, (long long)u.h * u.w);
      }
      uint8_t* cut = s.scratch.alloc<uint8_t>(cut_bytes);
      k = 0;
      for (int i = g0; i < g1; i++) {
        const DetUnit& u = units[(size_t)i];
        hd[i - g0] = u.ty < 0 ? nn::U8Page{P.pg[u.page].det_img, (long long)u.h * u.w, L0.h[i - g0].off}
                              : nn::U8Page{cut + ht[k++].cut_off, (long long)u.h * u.w, L0.h[i - g0].off};
      }
      RT_HIP_CHECK(hipMemcpyAsync(d_tiles, ht, (size_t)nt * sizeof(dt::TileDesc), hipMemcpyHostToDevice, s.st));
      ProfScope ps(&s.prof, s.st, "det_tile_cut");
      pp::det_tile_cut(s.st, d_tiles, nt, max_tile_pix, cut);
    } else {
      for (int i = g0; i < g1; i++)
        hd[i - g0] = nn::U8Page{P.pg[units[(size_t)i].page].det_img, (long long)units[(size_t)i].h * units[(size_t)i].w, L0.h[i - g0].off};
    }
    RT_HIP_CHECK(hipMemcpyAsync(dd, hd, (size_t)gn * sizeof(nn::U8Page), hipMemcpyHostToDevice, s.st));
    RunCtx c = s.ctx(&s.scratch);
    float* map;
    { ProfOuter po(&s.prof, s.st, "net/det"); map = s.sh->det->run_u8(c, dd, s.sh->cfg.det_scale, s.sh->cfg.det_mean, s.sh->cfg.det_std, L0); }
    if (nt == 0) {
      // keep the maps beyond the next group's scratch rewind; the last group's map is consumed by the DB post-processing
      // (same stream) before the classifier reuses the scratch arena, so it stays where the network left it
      float* keep = map;
      if (g1 < nu) {
        keep = s.arena.alloc<float>((size_t)L0.total);
        RT_HIP_CHECK(hipMemcpyAsync(keep, map, (size_t)L0.total * 4, hipMemcpyDeviceToDevice, s.st));
      }
      for (int i = g0; i < g1; i++) P.pg[units[(size_t)i].page].map = keep + L0.h[i - g0].off;
      checksum(keep, L0.total);
    } else {
      { ProfScope ps(&s.prof, s.st, "det_tile_stitch");
        pp::det_tile_stitch(s.st, d_tiles, nt, max_tile_pix, map); }
      for (int i = g0; i < g1; i++) {
        const DetUnit& u = units[(size_t)i];
        const long long px = (long long)u.h * u.w;
        float* m = map + L0.h[i - g0].off;
        if (u.ty >= 0) {   // (rt_debug_det_tiles: the tile's own map, at its place in plan order)
          if (P.tile_maps_out)
            RT_HIP_CHECK(hipMemcpyAsync(P.tile_maps_out + ((long long)u.ty * cols[(size_t)u.page].n() + u.tx) * px, m, (size_t)px * 4, hipMemcpyDeviceToHost, s.st));
          continue;
        }
        // an untiled page of a group that holds tiles: its own copy (the last group's stays in scratch) and its own checksum
        if (g1 < nu) {
          float* keep = s.arena.alloc<float>((size_t)px);
          RT_HIP_CHECK(hipMemcpyAsync(keep, m, (size_t)px * 4, hipMemcpyDeviceToDevice, s.st));
          m = keep;
        }
        P.pg[u.page].map = m;
        checksum(m, px);
      }
    }
    g0 = g1;
  }
  // the checksum is taken over the page maps: a tiled page's stitched map, never its tiles
  for (int i = 0; i < P.call.n_pages; i++) {
    if (!page_map[(size_t)i]) continue;
    checksum(page_map[(size_t)i], (long long)P.pg[i].det_h * P.pg[i].det_w);
  }
}
// ---- a5: DB post-processing of every page (on device; stream-ordered workspace reuse) ----
void db_post(rt_lane& s, Pipeline& P) {
  const int n = P.call.n_pages, mb = max_boxes_of(s.sh->cfg);
  // box lists and counts of all pages are contiguous: one pack launch + two copies bring them to the host
  pp::DbBox* d_boxes = s.arena.alloc<pp::DbBox>((size_t)mb * n);
  P.d_counts = s.arena.alloc<int>((size_t)2 * n);
  P.d_boxes_packed = s.arena.alloc<pp::DbBox>((size_t)mb * n);
  std::vector<pp::DbPageIn> in((size_t)n);
  for (int i = 0; i < n; i++) {
    const PageState& p = P.pg[i];
    const float* pred = p.map;
    if (P.call.det_map_override && P.call.det_map_override[i]) {
      if (P.call.mem == RT_MEM_HOST || P.call.mem == RT_MEM_STAGED_MAPS_HOST) {
        float* d = s.arena.alloc<float>((size_t)p.det_h * p.det_w);
        RT_HIP_CHECK(hipMemcpyAsync(d, P.call.det_map_override[i], (size_t)p.det_h * p.det_w * 4, hipMemcpyHostToDevice, s.st));
        pred = d;
      } else pred = P.call.det_map_override[i];
    }
    in[i] = pp::DbPageIn{pred, p.det_h, p.det_w, p.after_h, p.after_w};
  }
  ProfScope ps(&s.prof, s.st, "db_postprocess");
  db_post_enqueue(s, n, in.data(), d_boxes, P.d_counts);
  pp::pack_boxes(s.st, n, d_boxes, P.d_counts, mb, P.d_boxes_packed);
}
// ---- metadata round trip #1: box lists (a few KB per page); pixels and tensors stay on the device ----
void box_round_trip(rt_lane& s, Pipeline& P, rt_results& res) {
  const int n = P.call.n_pages;
  int* h_counts = s.pinned.alloc<int>((size_t)2 * n);
  RT_HIP_CHECK(hipMemcpyAsync(h_counts, P.d_counts, (size_t)2 * n * sizeof(int), hipMemcpyDeviceToHost, s.st));
  // (the map checksum partials ride to pinned memory with the box counts)
  std::vector<double*> h_sum(P.sum_parts.size());
  for (size_t g = 0; g < P.sum_parts.size(); g++) {
    h_sum[g] = s.pinned.alloc<double>((size_t)P.sum_counts[g]);
    RT_HIP_CHECK(hipMemcpyAsync(h_sum[g], P.sum_parts[g], (size_t)P.sum_counts[g] * 8, hipMemcpyDeviceToHost, s.st));
  }
  s.sync(); s.check_flags();
  int total_lines = 0;
  for (int i = 0; i < n; i++) {
    if (h_counts[2 * i + 1]) throw RtError(RT_ERR_CAPACITY, "DB post-processing work list overflow (raise max_boxes_per_page)");
    PageState& p = P.pg[i];
    p.n_boxes = std::min(std::max(h_counts[2 * i], 0), max_boxes_of(s.sh->cfg)); p.first_line = total_lines; total_lines += p.n_boxes;
  }
  if (total_lines > 0) {
    pp::DbBox* h_boxes = s.pinned.alloc<pp::DbBox>((size_t)total_lines);
    RT_HIP_CHECK(hipMemcpyAsync(h_boxes, P.d_boxes_packed, (size_t)total_lines * sizeof(pp::DbBox), hipMemcpyDeviceToHost, s.st));
    s.sync();
    for (PageState& p : P.pg) p.boxes = h_boxes + p.first_line;
  }
  for (size_t g = 0; g < P.sum_parts.size(); g++)
    for (int i = 0; i < P.sum_counts[g]; i++) res.det_checksum += h_sum[g][i];
  P.NL = total_lines; P.NLp = std::max(total_lines, 1);
  P.tok_off.assign((size_t)P.NL + 1, 0);
  if (P.call.cb)  // run_stream: the Det stage is complete here (session.rs:98)
    for (int i = 0; i < n; i++) { rt_results::Page page; page_boxes(P.pg[i], page, false); emit_stage(P.call, i, 0, page); }
}
// ---- rt_run_regions: instead of a2 .. a5 and round trip #1 -- the pages as they are, the boxes from the caller ----
void region_pages(rt_lane& s, Pipeline& P) {
  const PageCall& c = P.call;
  int total_lines = 0;
  for (int i = 0; i < c.n_pages; i++) total_lines += c.n_quads[i];
  P.region_boxes.resize((size_t)total_lines);
  total_lines = 0;
  for (int i = 0; i < P.call.n_pages; i++) {
    PageState& p = P.pg[i];
    p.ori_h = p.after_h = c.hs[i]; p.ori_w = p.after_w = c.ws[i]; p.det_h = p.det_w = 0;
    p.n_boxes = c.n_quads[i]; p.first_line = total_lines;
    p.raw = p.img = p.n_boxes > 0 ? page_on_device(s, c, i) : nullptr;   // (a page without regions is never read)
    p.det_img = nullptr; p.map = nullptr;
    for (int k = 0; k < p.n_boxes; k++) {
      pp::DbBox& b = P.region_boxes[(size_t)total_lines + k];
      memcpy(b.pts, c.quads[i] + 8 * k, 32); b.score = 1.0f; b.key = 0;
    }
    p.boxes = P.region_boxes.data() + total_lines;
    total_lines += p.n_boxes;
  }
  P.NL = total_lines; P.NLp = std::max(total_lines, 1);
  P.tok_off.assign((size_t)P.NL + 1, 0);
}
// ---- a6: crop plan over every page's boxes, the crops warped when there are any ----
// Resized (the reference): box k in after-resize_both coordinates, cut from the resized page.  Original / regions: the quad the
// results report (page_boxes: after scale_and_clip, or the caller's clamped quad), cut from the caller's page; everything
// downstream reads the plan, so the crop size, rotate270, the homography and the cls / rec ordering follow that quad.
void crop_stage(rt_lane& s, Pipeline& P) {
  for (const PageState& p : P.pg) {
    if (!P.crop_original) {
      for (int k = 0; k < p.n_boxes; k++) plan_crop(P.plan, p.img, p.after_h, p.after_w, p.boxes[k].pts);
      continue;
    }
    rt_results::Page B;
    page_boxes(p, B, P.call.regions());
    for (int k = 0; k < p.n_boxes; k++) plan_crop(P.plan, p.raw, p.ori_h, p.ori_w, &B.boxes[8 * (size_t)k]);
  }
  if (P.NL > 0) P.pool = warp_planned_crops(s, P.plan, &P.d_refs, P.crop_original);
}
// ---- a8 + a9: angle classifier over every crop --------------------------------------
// (cls_processor.rs:127-172: batches of 6 sorted by aspect; the classifier is per-crop independent, so batch composition does
//  not change any value)
void cls_stage(rt_lane& s, Pipeline& P) {
  const int ch = s.sh->cfg.cls_image_shape[1], cw = s.sh->cfg.cls_image_shape[2];
  P.d_meta.view(s.arena.alloc<int>((size_t)4 * P.NLp), P.NLp);
  const int CG = 2048;
  for (int c0 = 0; c0 < P.NL; c0 += CG) {
    int cn = std::min(CG, P.NL - c0);
    s.scratch.rewind();
    pp::LineDesc* hl = s.pinned.alloc<pp::LineDesc>(cn);
    int* hrow = s.pinned.alloc<int>(cn);
    for (int k = 0; k < cn; k++) {
      const pp::CropRef& r = P.plan.refs[c0 + k];
      hl[k] = line_desc(r, r.h, r.w, ch, cw); hl[k].out_off = (long long)k * ch * cw * 4;
      hrow[k] = c0 + k;
    }
    pp::LineDesc* dl = s.scratch.alloc<pp::LineDesc>(cn);
    int* drow = s.scratch.alloc<int>(cn);
    RT_HIP_CHECK(hipMemcpyAsync(dl, hl, (size_t)cn * sizeof(pp::LineDesc), hipMemcpyHostToDevice, s.st));
    RT_HIP_CHECK(hipMemcpyAsync(drow, hrow, (size_t)cn * 4, hipMemcpyHostToDevice, s.st));
    float* x = s.scratch.alloc<float>((size_t)cn * ch * cw * 4);
    { ProfScope ps(&s.prof, s.st, "resize_norm");
      pp::resize_norm(s.st, dl, cn, ch, cw, P.pool, 0, x, s.d_flags); }
    Level L0 = make_level(uniform_hw(cn, ch, cw));
    RunCtx c = s.ctx(&s.scratch);
    float* probs;
    { ProfOuter po(&s.prof, s.st, "net/cls"); probs = s.sh->cls->run(c, x, L0); }
    ProfScope ps(&s.prof, s.st, "cls_post_rotate");
    pp::cls_post_rotate(s.st, probs, drow, cn, s.sh->cfg.cls_thresh, P.d_refs, P.pool, P.plan.max_pix, P.d_meta.label, P.d_meta.cscore);
  }
}
// ---- rec flip (rec_flip.h): which lines are read both ways.  With 0 < cls_below <= 1 that takes the classifier scores: one copy
// of NL floats and one lane sync, only then; above 1 every line is, without a sync.  A call without a both-ways line allocates nothing.
void flip_plan(rt_lane& s, Pipeline& P) {
  const float below = P.call.set.flip_cls_below;
  if (!(below > 0.0f) || P.NL == 0) return;
  bool any = false;
  if (rf::every_line(below)) { P.both.assign((size_t)P.NL, 1); any = true; }
  else {
    float* h = s.pinned.alloc<float>((size_t)P.NL);
    RT_HIP_CHECK(hipMemcpyAsync(h, P.d_meta.cscore, (size_t)P.NL * sizeof(float), hipMemcpyDeviceToHost, s.st));
    s.sync();
    P.both.resize((size_t)P.NL);
    for (int l = 0; l < P.NL; l++) { P.both[(size_t)l] = rf::both_ways(h[l], below) ? 1 : 0; any = any || P.both[(size_t)l]; }
  }
  if (!any) { P.both.clear(); return; }
  P.flipo.alloc(s, P.NLp); P.flips.alloc(s, (size_t)2 * P.NLp);
  RT_HIP_CHECK(hipMemsetAsync(P.flipo.d, 0, (size_t)P.NLp * sizeof(int), s.st));
  RT_HIP_CHECK(hipMemsetAsync(P.flips.d, 0, (size_t)2 * P.NLp * sizeof(float), s.st));
}
// ---- a10: rec plan: per page, order by h/w descending (stable), chunks of batch_num, running max_wh_ratio ----
void rec_plan(rt_lane& s, Pipeline& P) {
  const int rh = s.sh->cfg.rec_image_shape[1], rw = s.sh->cfg.rec_image_shape[2];
  const std::vector<pp::CropRef>& refs = P.plan.refs;
  P.lines.resize((size_t)P.NL); P.line_W.resize((size_t)P.NL);
  for (const PageState& p : P.pg) {
    int nb = p.n_boxes, f = p.first_line;
    std::vector<int> order((size_t)nb);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
      double ra = (double)refs[f + a].h / (double)refs[f + a].w;
      double rb = (double)refs[f + b].h / (double)refs[f + b].w;
      return ra > rb;  // Reverse(OrderedFloat(ori_ratio))
    });
    float max_wh_ratio = (float)rw / (float)rh;
    for (int s0 = 0; s0 < nb; s0 += s.sh->cfg.rec_batch_num) {
      int s1 = std::min(nb, s0 + s.sh->cfg.rec_batch_num);
      for (int k = s0; k < s1; k++) {
        const pp::CropRef& r = refs[f + order[k]];
        float wh = (float)r.w / (float)r.h;
        if (wh > max_wh_ratio) max_wh_ratio = wh;
      }
      int W = gm::resize_norm_width(rh, rw, max_wh_ratio);
      for (int k = s0; k < s1; k++) {
        int li = f + order[k];
        const pp::CropRef& r = refs[li];
        P.lines[li] = line_desc(r, r.h, r.w, rh, W); P.line_W[li] = W;
      }
    }
  }
  for (int l = 0; l < P.NL; l++) P.tok_off[l + 1] = P.tok_off[l] + RecNet::tokens_for_width(P.line_W[l]);
}
// line li as the rec network saw it (word_boxes.h): what k_word_boxes and the keyword spans' quads map columns through
wb::WordGeom word_geom(const Pipeline& P, int li) {
  const pp::CropRef& r = P.plan.refs[li];
  const pp::CropDesc& cd = P.plan.descs[li];
  wb::WordGeom g;
  g.T = (int)(P.tok_off[li + 1] - P.tok_off[li]); g.W = P.line_W[li]; g.resized_w = P.lines[li].resized_w;
  g.w_c = r.w; g.h_c = r.h; g.rot270 = cd.rot; g.w = cd.w; g.h = cd.h;
  g.cw = P.plan.dims[li].cw; g.ch = P.plan.dims[li].ch;
  memcpy(g.inv, cd.inv, sizeof g.inv);
  return g;
}
// ---- the rec network over ONE rec group: whole lines, or windows (rec_windows.h) --------
// x = the group's line tensors as resize_norm wrote them (NHWC-4, rh rows, W[k] columns, concatenated).  idx / prob receive the
// lines' rows, *z5 (when asked for) their head-input rows, Lt their token level on the device: exactly what RecModel::run leaves.
// A group without a windowed line IS RecModel::run on the lines, what it was before windows existed: the same launches, the same
// bits, nothing allocated.  With one, every line becomes its units (a whole line: one unit that owns all its rows):
// k_rec_window_cut copies the units' column ranges into ragged unit tensors, the network runs once over the units as its
// "lines" with idx / prob / z5 in scratch, and k_rec_window_stitch gathers the owned rows into the line rows.
// taps (rt_debug_rec_windows): host arrays that receive every unit's rows in unit order, each optional.
struct RecWindowTaps { int32_t* unit_idx = nullptr; float* unit_prob = nullptr; float* unit_z5 = nullptr; };
void rec_group_net(rt_lane& s, const float* x, int rh, const int* W, int ln, int window, int overlap, int* idx, float* prob,
                   const float** z5, Level& Lt, const RecWindowTaps* taps = nullptr) {
  static_assert(rw::Z5_D == 120, "a z5 row is SvtrCore::D floats");
  RunCtx c = s.ctx(&s.scratch);
  const auto tap = [&](const int* d_idx, const float* d_prob, const float* d_z5, long long rows) {
    if (!taps || rows <= 0) return;
    if (taps->unit_idx) RT_HIP_CHECK(hipMemcpyAsync(taps->unit_idx, d_idx, (size_t)rows * 4, hipMemcpyDeviceToHost, s.st));
    if (taps->unit_prob) RT_HIP_CHECK(hipMemcpyAsync(taps->unit_prob, d_prob, (size_t)rows * 4, hipMemcpyDeviceToHost, s.st));
    if (taps->unit_z5 && d_z5) RT_HIP_CHECK(hipMemcpyAsync(taps->unit_z5, d_z5, (size_t)rows * rw::Z5_D * 4, hipMemcpyDeviceToHost, s.st));
  };
  std::vector<std::pair<int, int>> hw;
  bool windowed = false;
  for (int k = 0; k < ln; k++) { hw.push_back({rh, W[k]}); windowed = windowed || rw::line_windowed(W[k], window); }
  if (!windowed) {
    Level L0 = make_level(hw);
    { ProfOuter po(&s.prof, s.st, "net/rec");
      s.sh->rec->run(c, x, L0, Lt, idx, prob, z5); }  // fused CTC head: logits never reach HBM
    tap(idx, prob, z5 ? *z5 : nullptr, Lt.total);
    return;
  }
  int nu = 0;
  for (int k = 0; k < ln; k++) nu += rw::units(W[k], window, overlap);
  // the units' descriptors through pinned into scratch, as the det tiles' go
  rw::UnitDesc* hu = s.pinned.alloc<rw::UnitDesc>((size_t)nu);
  rw::UnitDesc* du = s.scratch.alloc<rw::UnitDesc>((size_t)nu);
  std::vector<std::pair<int, int>> uhw, thw;
  long long line_px = 0, unit_px = 0, line_rows = 0, unit_rows = 0;
  int max_w = 0, max_own = 0, u = 0;
  for (int k = 0; k < ln; k++) {
    const rw::Plan p = rw::plan(W[k], window, overlap);
    if (p.T != RecNet::tokens_for_width(W[k])) throw RtError(RT_ERR_BACKEND, "rec windows: rw::tokens and RecNet::tokens_for_width disagree");
    for (int i = 0; i < p.n(); i++) {
      rw::UnitDesc& d = hu[u++];
      d.src_off = line_px; d.dst_off = unit_px; d.unit_row = unit_rows; d.line_row = line_rows;
      d.line_w = W[k]; d.x0 = p.origin[(size_t)i]; d.w = p.width[(size_t)i];
      d.m = d.x0 / rw::STEP; d.t0 = p.own0(i); d.t1 = p.bound[(size_t)i];
      const int Tu = RecNet::tokens_for_width(d.w);
      // (what the kernels rely on: the unit's columns inside its line, its owned steps inside its own rows and the line's)
      if (d.x0 < 0 || d.w < rw::STEP || d.x0 + d.w > W[k] || d.t0 < d.m || d.t1 < d.t0 || d.t1 - d.m > Tu || d.t1 > p.T)
        throw RtError(RT_ERR_BACKEND, "rec windows: a unit lies outside its line");
      uhw.push_back({rh, d.w});
      unit_px += (long long)rh * d.w; unit_rows += Tu;
      max_w = std::max(max_w, d.w); max_own = std::max(max_own, d.t1 - d.t0);
    }
    thw.push_back({1, p.T});
    line_px += (long long)rh * W[k]; line_rows += p.T;
  }
  RT_HIP_CHECK(hipMemcpyAsync(du, hu, (size_t)nu * sizeof(rw::UnitDesc), hipMemcpyHostToDevice, s.st));
  float* xu = s.scratch.alloc<float>((size_t)unit_px * 4);
  { ProfScope ps(&s.prof, s.st, "rec_window_cut");
    pp::rec_window_cut(s.st, du, nu, rh, max_w, x, xu); }
  int* u_idx = s.scratch.alloc<int>((size_t)unit_rows); float* u_prob = s.scratch.alloc<float>((size_t)unit_rows);
  float* l_z5 = z5 ? s.scratch.alloc<float>((size_t)line_rows * rw::Z5_D) : nullptr;
  const float* u_z5 = nullptr;
  Level Lu0 = make_level(uhw), Ltu;
  { ProfOuter po(&s.prof, s.st, "net/rec");
    s.sh->rec->run(c, xu, Lu0, Ltu, u_idx, u_prob, z5 ? &u_z5 : nullptr); }
  if (Ltu.total != unit_rows) throw RtError(RT_ERR_SHAPE, "token count mismatch");
  { ProfScope ps(&s.prof, s.st, "rec_window_stitch");
    pp::rec_window_stitch(s.st, du, nu, max_own, u_idx, u_prob, u_z5, idx, prob, l_z5); }
  if (z5) *z5 = l_z5;
  // the LINES' token level, as RecModel::run would have left it: {first row, 1, T} per line
  Lt = make_level(thw);
  upload_levels(c, {&Lt});
  tap(u_idx, u_prob, u_z5, unit_rows);
}
// ---- ONE rec group with a both-ways line (rec_flip.h) ----------------------------------
// lines / W / both: the group's ln lines as the rec plan left them (crop_off into pool) and their flags, at least one set.  The
// group's tensor is the lines followed by the view-1 copies of the flagged lines: k_rec_flip_rotate writes their crops rotated
// into a second pool region in scratch, resize_norm reads the pool for the lines and that region for the copies, and
// rec_group_net runs ONCE over the views with idx / prob / z5 in scratch (rec windows apply to each view as to any line).
// k_ctc_decode over the views' rows gives each its kept count and greedy score; the views' leading rows are the lines' view 0 in
// the lines' own layout, so one block copy brings them to idx / prob and the z5 prefix is the lines' z5; k_rec_flip_select then
// writes the flagged lines' outcome and scores at slot0 + k and copies a chosen view's rows over the line's.  Lt: the LINES'
// token level, as RecModel::run would have left it.  taps (rt_debug_rec_flip): host arrays, each optional.
struct RecFlipTaps { int32_t* view_idx = nullptr; float* view_prob = nullptr; float* view_z5 = nullptr; int32_t* view_ntok = nullptr; float* view_score = nullptr; };
void rec_group_flip(rt_lane& s, const uint8_t* pool, const pp::LineDesc* lines, const int* W, const uint8_t* both, int ln, int slot0,
                    int rh, int window, int overlap, int* idx, float* prob, const float** z5, Level& Lt, int* outcome, float* scores,
                    const RecFlipTaps* taps = nullptr) {
  int nf = 0;
  for (int k = 0; k < ln; k++) nf += both[k] ? 1 : 0;
  const int nv = ln + nf;
  rf::FlipCrop* hc = s.pinned.alloc<rf::FlipCrop>((size_t)nf);
  rf::SelectDesc* hs = s.pinned.alloc<rf::SelectDesc>((size_t)nf);
  pp::LineDesc* hl = s.pinned.alloc<pp::LineDesc>((size_t)nv);
  std::vector<int> Wv((size_t)nv);
  std::vector<std::pair<int, int>> thw;
  long long off = 0, rows = 0, fpix = 0;
  int maxW = 0, maxWf = 0, maxT = 0;
  for (int k = 0; k < ln; k++) {
    hl[k] = lines[k]; hl[k].out_off = off * 4;
    off += (long long)rh * W[k]; Wv[(size_t)k] = W[k]; maxW = std::max(maxW, W[k]);
    const int T = RecNet::tokens_for_width(W[k]);
    thw.push_back({1, T}); rows += T;
  }
  long long vrows = rows, row0 = 0;
  for (int k = 0, f = 0; k < ln; k++) {
    const int T = RecNet::tokens_for_width(W[k]);
    if (both[k]) {
      const long long npix = (long long)lines[k].h * lines[k].w;
      if (npix <= 0) throw RtError(RT_ERR_BACKEND, "rec flip: an empty crop");
      hc[f] = rf::FlipCrop{lines[k].crop_off, fpix * 3, fpix, npix};
      pp::LineDesc& v = hl[ln + f];
      v = lines[k]; v.crop_off = fpix * 3; v.out_off = off * 4;   // (the same thumbnail and padded width, read from the second region)
      off += (long long)rh * W[k]; Wv[(size_t)(ln + f)] = W[k]; maxWf = std::max(maxWf, W[k]);
      hs[f] = rf::SelectDesc{row0, vrows, row0, k, ln + f, T, slot0 + k};
      fpix += npix; vrows += T; maxT = std::max(maxT, T); f++;
    }
    row0 += T;
  }
  rf::FlipCrop* dc = s.scratch.alloc<rf::FlipCrop>((size_t)nf);
  rf::SelectDesc* ds = s.scratch.alloc<rf::SelectDesc>((size_t)nf);
  pp::LineDesc* dl = s.scratch.alloc<pp::LineDesc>((size_t)nv);
  RT_HIP_CHECK(hipMemcpyAsync(dc, hc, (size_t)nf * sizeof(rf::FlipCrop), hipMemcpyHostToDevice, s.st));
  RT_HIP_CHECK(hipMemcpyAsync(ds, hs, (size_t)nf * sizeof(rf::SelectDesc), hipMemcpyHostToDevice, s.st));
  RT_HIP_CHECK(hipMemcpyAsync(dl, hl, (size_t)nv * sizeof(pp::LineDesc), hipMemcpyHostToDevice, s.st));
  uint8_t* flipped = s.scratch.alloc<uint8_t>((size_t)fpix * 3);
  { ProfScope ps(&s.prof, s.st, "rec_flip_rotate");
    pp::rec_flip_rotate(s.st, dc, nf, fpix, pool, flipped); }
  float* x = s.scratch.alloc<float>((size_t)off * 4);
  { ProfScope ps(&s.prof, s.st, "resize_norm");
    pp::resize_norm(s.st, dl, ln, rh, maxW, pool, 0, x, s.d_flags); }
  { ProfScope ps(&s.prof, s.st, "resize_norm");
    pp::resize_norm(s.st, dl + ln, nf, rh, maxWf, flipped, 0, x, s.d_flags); }
  int* v_idx = s.scratch.alloc<int>((size_t)std::max<long long>(vrows, 1)); float* v_prob = s.scratch.alloc<float>((size_t)std::max<long long>(vrows, 1));
  const float* v_z5 = nullptr;
  Level Lv;
  rec_group_net(s, x, rh, Wv.data(), nv, window, overlap, v_idx, v_prob, z5 ? &v_z5 : nullptr, Lv);
  if (Lv.total != vrows) throw RtError(RT_ERR_SHAPE, "token count mismatch");
  // the views' (kept tokens, greedy score): k_ctc_decode itself, its tokens into scratch
  int* v_tok = s.scratch.alloc<int>((size_t)std::max<long long>(vrows, 1));
  int* v_ntok = s.scratch.alloc<int>((size_t)nv); float* v_score = s.scratch.alloc<float>((size_t)nv);
  { ProfScope ps(&s.prof, s.st, "rec_flip_score");
    pp::ctc_decode(s.st, v_idx, v_prob, Lv.d, nv, v_tok, v_ntok, v_score); }
  if (taps && vrows > 0) {   // (the views' rows as the network left them: before the select moves a taken view 1 into the z5 prefix)
    if (taps->view_idx) RT_HIP_CHECK(hipMemcpyAsync(taps->view_idx, v_idx, (size_t)vrows * 4, hipMemcpyDeviceToHost, s.st));
    if (taps->view_prob) RT_HIP_CHECK(hipMemcpyAsync(taps->view_prob, v_prob, (size_t)vrows * 4, hipMemcpyDeviceToHost, s.st));
    if (taps->view_z5 && v_z5) RT_HIP_CHECK(hipMemcpyAsync(taps->view_z5, v_z5, (size_t)vrows * rw::Z5_D * 4, hipMemcpyDeviceToHost, s.st));
  }
  if (taps && taps->view_ntok) RT_HIP_CHECK(hipMemcpyAsync(taps->view_ntok, v_ntok, (size_t)nv * 4, hipMemcpyDeviceToHost, s.st));
  if (taps && taps->view_score) RT_HIP_CHECK(hipMemcpyAsync(taps->view_score, v_score, (size_t)nv * 4, hipMemcpyDeviceToHost, s.st));
  if (rows > 0) {
    RT_HIP_CHECK(hipMemcpyAsync(idx, v_idx, (size_t)rows * sizeof(int), hipMemcpyDeviceToDevice, s.st));
    RT_HIP_CHECK(hipMemcpyAsync(prob, v_prob, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s.st));
  }
  { ProfScope ps(&s.prof, s.st, "rec_flip_select");
    pp::rec_flip_select(s.st, ds, nf, maxT, v_ntok, v_score, v_idx, v_prob, const_cast<float*>(v_z5), idx, prob, outcome, scores); }
  if (z5) *z5 = v_z5;
  Lt = make_level(thw);
  RunCtx c = s.ctx(&s.scratch);
  upload_levels(c, {&Lt});
}
// ---- a11 + a12: rec network + CTC decode in launch groups (+ word boxes) --------------
void rec_groups(rt_lane& s, Pipeline& P) {
  const CallSettings& set = P.call.set;
  const int rh = s.sh->cfg.rec_image_shape[1];
  const size_t ntok = (size_t)std::max<long long>(P.tok_off[P.NL], 1);
  int* d_idx = s.arena.alloc<int>(ntok); float* d_prob = s.arena.alloc<float>(ntok);
  // rec_return_candidates = K: per token slot its time step and K candidates, in one block behind the tokens ([ntok] tokens |
  // [ntok] time steps | [ntok][K] candidates), so that the one copy that brings the tokens home brings them too
  const int cand_k = s.sh->cfg.rec_return_candidates;
  P.d_tok = s.arena.alloc<int>(ntok * (cand_k > 0 ? 2 + 2 * (size_t)cand_k : 1));
  if (cand_k > 0) { P.d_ccol = P.d_tok + ntok; P.d_cands = reinterpret_cast<cc::Cand*>(P.d_ccol + ntok); }
  // rec_return_word_box: word count per line, words at the lines' token offsets, the kept columns (k_word_boxes' scratch)
  int* d_wcol = nullptr;
  if (s.sh->cfg.rec_return_word_box) {
    P.d_wcount = s.arena.alloc<int>(P.NLp); P.d_words = s.arena.alloc<wb::Word>(ntok); d_wcol = s.arena.alloc<int>(ntok);
  }
  if (P.any.lexicon) { P.lexm.alloc(s, (size_t)P.NLp * lx::MATCHES); P.lexn.alloc(s, P.NLp); }
  // lexicon snap (ctc_lexicon_align.h): a line snaps only where its lexicon has min_posterior > 0
  if (std::any_of(P.line_opts.begin(), P.line_opts.end(), [&](const RecLineOpts& o) { return o.lexicon > 0 && s.sh->lexicons->snap[o.lexicon - 1] > 0.0f; })) {
    P.lexs.alloc(s, P.NLp);   // (zeroed: the lexicon lines of a group without a snap-enabled line are never written)
    RT_HIP_CHECK(hipMemsetAsync(P.lexs.d, 0, (size_t)P.NLp * sizeof(int), s.st));
  }
  if (P.any.pattern) P.pat.alloc(s, (size_t)4 * P.NLp);
  if (P.any.keywords) { P.kwh.alloc(s, (size_t)P.NLp * kw::HITS); P.kwn.alloc(s, P.NLp); }
  if (set.beam_b > 0) { P.bmn.alloc(s, P.NLp); P.bmrec.alloc(s, (size_t)P.NLp * set.beam_n); P.bmtok.alloc(s, ntok * (size_t)set.beam_n); }
  if (set.fused()) P.bmlm.alloc(s, (size_t)P.NLp * set.beam_n);
  if (set.worded()) P.bmvc.alloc(s, (size_t)P.NLp * set.beam_n);
  static const long long REC_GROUP_PX = getenv("RT_REC_GROUP_PX") ? atoll(getenv("RT_REC_GROUP_PX")) : (long long)24000000;  // measured sweet spot (profiles/README.md)
  for (int l0 = 0; l0 < P.NL;) {
    // (a windowed line is charged with its units' pixels, rec_windows.h: what the network is run on; a both-ways line, rec_flip.h,
    //  twice: both views run in the group's one pass)
    const int l1 = group_end(l0, P.NL, 0, REC_GROUP_PX, [&](int l) {
      return (!P.both.empty() && P.both[(size_t)l] ? 2 : 1) * (long long)rh * rw::unit_columns(P.line_W[l], set.rec_window, set.rec_overlap);
    });
    const int ln = l1 - l0;
    // a group without a both-ways line takes the path it took before rec flip existed: nothing new is launched or allocated
    const bool flip = !P.both.empty() && std::any_of(P.both.begin() + l0, P.both.begin() + l1, [](uint8_t b) { return b != 0; });
    s.scratch.rewind();
    float* x = nullptr;
    if (!flip) {
      pp::LineDesc* hl = s.pinned.alloc<pp::LineDesc>(ln);
      long long off = 0; int maxW = 0;
      for (int k = 0; k < ln; k++) {
        hl[k] = P.lines[l0 + k];
        hl[k].out_off = off * 4;
        off += (long long)rh * P.line_W[l0 + k];
        maxW = std::max(maxW, P.line_W[l0 + k]);
      }
      pp::LineDesc* dl = s.scratch.alloc<pp::LineDesc>(ln);
      RT_HIP_CHECK(hipMemcpyAsync(dl, hl, (size_t)ln * sizeof(pp::LineDesc), hipMemcpyHostToDevice, s.st));
      x = s.scratch.alloc<float>((size_t)off * 4);
      { ProfScope ps(&s.prof, s.st, "resize_norm");
        pp::resize_norm(s.st, dl, ln, rh, maxW, P.pool, 0, x, s.d_flags); }
    }
    Level Lt;
    // (the token count per line only depends on the widths, so the offsets are known before the net runs)
    const long long t0 = P.tok_off[l0];
    const rt_lexicons& X = *s.sh->lexicons;
    const rt_keywords& KW = *s.sh->keywords;
    const RecTailPlan tail = rec_tail_plan(P.tok_off.data(), l0, l1, P.line_opts.data(), RecStores{&X.tb, X.snap, &s.sh->patterns->tb, &KW.tb},
                                           set.beam_b, set.beam_n);
    const std::string refused = tail.refusal(set.beam_b);
    if (!refused.empty()) throw RtError(RT_ERR_CAPACITY, refused);
    const float* z5 = nullptr;   // the head's input, for the candidates', the charsets', the lexicons', the keywords' and the beams' logits
    if (!flip) rec_group_net(s, x, rh, P.line_W.data() + l0, ln, set.rec_window, set.rec_overlap, d_idx + t0, d_prob + t0, tail.needs_z5(cand_k) ? &z5 : nullptr, Lt);
    else rec_group_flip(s, P.pool, P.lines.data() + l0, P.line_W.data() + l0, P.both.data() + l0, ln, l0, rh, set.rec_window, set.rec_overlap,
                        d_idx + t0, d_prob + t0, tail.needs_z5(cand_k) ? &z5 : nullptr, Lt, P.flipo.d, P.flips.d);
    if (Lt.total != tail.rows) throw RtError(RT_ERR_SHAPE, "token count mismatch");
    rt_lane::WordBoxes words{};
    if (s.sh->cfg.rec_return_word_box) {
      pp::WordLineDesc* hwl = s.pinned.alloc<pp::WordLineDesc>(ln);
      for (int k = 0; k < ln; k++) {
        const int li = l0 + k;
        hwl[k].tok_off = P.tok_off[li] - t0;
        hwl[k].g = word_geom(P, li);
      }
      words = {hwl, P.d_meta.label + l0, P.d_meta.cscore + l0, d_wcol + t0, P.d_wcount + l0, P.d_words + t0, P.flipo.d ? P.flipo.d + l0 : nullptr};
    }
    rt_lane::RecTail t;
    t.z5 = z5; t.idx = d_idx + t0; t.prob = d_prob + t0; t.lines = Lt.d; t.n_lines = ln;
    t.tok = P.d_tok + t0; t.ntok = P.d_meta.ntok + l0; t.rscore = P.d_meta.rscore + l0;
    if (words.h_lines) t.wb = &words;
    t.charsets = {s.sh->charsets->d_masks, s.sh->charsets->words};
    t.lexicon.d = X.d; t.lexicon.matches = P.lexm.d; t.lexicon.n = P.lexn.d; t.lexicon.d_min_post = X.d_snap; t.lexicon.snapped = P.lexs.d;
    t.pattern.d = s.sh->patterns->d;
    if (P.pat.d) {   // matched | vit | logprob | free_logprob
      float* f = reinterpret_cast<float*>(P.pat.d);
      t.pattern.matched = P.pat.d; t.pattern.vit = f + P.NLp; t.pattern.logprob = f + 2 * (size_t)P.NLp; t.pattern.free_logprob = f + 3 * (size_t)P.NLp;
    }
    t.keywords.d = KW.d; t.keywords.d_min = KW.d_min; t.keywords.hits = P.kwh.d; t.keywords.n = P.kwn.d;
    t.beam.b = set.beam_b; t.beam.n = set.beam_n; t.beam.count = P.bmn.d; t.beam.recs = P.bmrec.d;
    if (P.bmtok.d) t.beam.tok = P.bmtok.d + t0 * set.beam_n;
    if (set.fused()) { t.beam.fused = true; t.beam.fu = lm::Fusion{s.sh->lms->dev[(size_t)set.lm], set.lm_alpha, set.lm_beta}; t.beam.lms = P.bmlm.d; }
    if (set.worded()) { t.beam.worded = true; t.beam.wc = vc::Constraint{s.sh->vocabs->dev[(size_t)set.beam_vocab], set.vocab_gamma}; t.beam.vocs = P.bmvc.d; }
    t.cand.k = cand_k;
    if (cand_k > 0) { t.cand.col = P.d_ccol + t0; t.cand.cands = P.d_cands + t0 * cand_k; }
    s.rec_tail(tail, s.sh->rec->core(), t);
    l0 = l1;
  }
}
// ---- metadata round trip #2: labels, scores, token ids (and the words) ---------------
void line_round_trip(rt_lane& s, Pipeline& P) {
  const long long total_tok = P.tok_off[P.NL];
  // per-line results come back in two copies into pinned memory: the metadata block and the tokens
  P.h_meta.view(s.pinned.alloc<int>((size_t)4 * P.NLp), P.NLp);
  // (with rec_return_candidates = K the tokens' block also holds their time steps and candidates: rec_groups)
  const size_t nt = (size_t)std::max<long long>(total_tok, 1), K = (size_t)s.sh->cfg.rec_return_candidates;
  const size_t tok_words = nt * (K > 0 ? 2 + 2 * K : 1);
  P.h_tokens = s.pinned.alloc<int>(tok_words);
  if (K > 0) { P.h_ccol = P.h_tokens + nt; P.h_cands = reinterpret_cast<cc::Cand*>(P.h_ccol + nt); }
  RT_HIP_CHECK(hipMemcpyAsync(P.h_meta.label, P.d_meta.label, (size_t)4 * P.NLp * sizeof(int), hipMemcpyDeviceToHost, s.st));
  if (total_tok > 0) RT_HIP_CHECK(hipMemcpyAsync(P.h_tokens, P.d_tok, tok_words * 4, hipMemcpyDeviceToHost, s.st));
  if (s.sh->cfg.rec_return_word_box) {   // (the words ride with the tokens: same round trip)
    P.h_wcount = s.pinned.alloc<int>(P.NLp);
    P.h_words = s.pinned.alloc<wb::Word>((size_t)std::max<long long>(total_tok, 1));
    RT_HIP_CHECK(hipMemcpyAsync(P.h_wcount, P.d_wcount, (size_t)P.NL * sizeof(int), hipMemcpyDeviceToHost, s.st));
    if (total_tok > 0) RT_HIP_CHECK(hipMemcpyAsync(P.h_words, P.d_words, (size_t)total_tok * sizeof(wb::Word), hipMemcpyDeviceToHost, s.st));
  }
  // (and what the lexicons, the snap, the patterns, the keywords and the beams left, where the call has them)
  P.lexm.fetch(s.st); P.lexn.fetch(s.st); P.lexs.fetch(s.st); P.pat.fetch(s.st); P.kwh.fetch(s.st); P.kwn.fetch(s.st);
  P.bmn.fetch(s.st); P.bmrec.fetch(s.st); P.bmtok.fetch(s.st); P.bmlm.fetch(s.st); P.bmvc.fetch(s.st);
  P.flipo.fetch(s.st); P.flips.fetch(s.st);
  s.sync(); s.check_flags();
}
// ---- results (session.rs:94-105) ----------------------------------------------------
void results(const rt_session& s, const Pipeline& P, rt_results& res) {
  static const uint16_t LABELS[2] = {0, 180};
  const LineMeta& m = P.h_meta;
  for (int i = 0; i < P.call.n_pages; i++) {
    rt_results::Page& R = res.pages[i];
    const PageState& p = P.pg[i];
    int nb = p.n_boxes;
    page_boxes(p, R, P.call.regions());
    R.cls_labels.resize(nb); R.cls_scores.resize(nb); R.rec_scores.resize(nb); R.tokens.resize(nb); R.text.resize(nb);
    R.rec_units.resize(nb);
    for (int k = 0; k < nb; k++) R.rec_units[k] = rw::units(P.line_W[p.first_line + k], P.call.set.rec_window, P.call.set.rec_overlap);
    if (P.flipo.h) {   // rec flip: a line read one way reports 0 (its slots were never written)
      R.flip_outcome.assign((size_t)nb, 0); R.flip_scores.assign((size_t)2 * nb, 0.0f);
      for (int k = 0; k < nb; k++) {
        const int li = p.first_line + k;
        if (!P.both[(size_t)li]) continue;
        R.flip_outcome[k] = P.flipo.h[li] == rf::TOOK_1 ? rf::TOOK_1 : rf::KEPT_0;
        R.flip_scores[2 * (size_t)k] = P.flips.h[2 * (size_t)li]; R.flip_scores[2 * (size_t)k + 1] = P.flips.h[2 * (size_t)li + 1];
      }
    }
    for (int k = 0; k < nb; k++) {
      int li = p.first_line + k;
      R.cls_labels[k] = LABELS[m.label[li] ? 1 : 0]; R.cls_scores[k] = m.cscore[li]; R.rec_scores[k] = m.rscore[li];
      R.tokens[k].assign(P.h_tokens + P.tok_off[li], P.h_tokens + P.tok_off[li] + m.ntok[li]);
      std::string& t = R.text[k];
      t.reserve(R.tokens[k].size() * 3);  // CJK dictionary entries are 3 UTF-8 bytes
      for (int id : R.tokens[k]) t += s.dict[(size_t)id];
    }
    if (const int K = s.cfg.rec_return_candidates) {
      R.cand_k = K; R.cand_off.assign((size_t)nb + 1, 0);
      for (int k = 0; k < nb; k++) R.cand_off[k + 1] = R.cand_off[k] + (uint32_t)m.ntok[p.first_line + k];
      R.cand_cols.resize(R.cand_off[nb]); R.cands.resize((size_t)R.cand_off[nb] * K);
      for (int k = 0; k < nb; k++) {
        const long long o = P.tok_off[p.first_line + k];
        const size_t n = (size_t)m.ntok[p.first_line + k];
        if (n == 0) continue;
        memcpy(&R.cand_cols[R.cand_off[k]], P.h_ccol + o, n * sizeof(int32_t));
        memcpy(&R.cands[(size_t)R.cand_off[k] * K], P.h_cands + o * K, n * K * sizeof(cc::Cand));
      }
    }
    if (P.any.lexicon) {   // rec lexicons: a line without one has 0 matches (its device slots were never written)
      R.lex_id.assign((size_t)nb, 0); R.lex_n.assign((size_t)nb, 0); R.lex_matches.assign((size_t)nb * lx::MATCHES, lx::Match{0, 0.0f, 0.0f});
      if (P.lexs.h) R.lex_snapped.assign((size_t)nb, 0);
      for (int k = 0; k < nb; k++) {
        const int li = p.first_line + k;
        if (P.line_opts[li].lexicon <= 0) continue;
        if (P.lexs.h) R.lex_snapped[k] = P.lexs.h[li] == 1 ? 1 : 0;
        R.lex_id[k] = P.line_opts[li].lexicon;
        R.lex_n[k] = std::min(std::max(P.lexn.h[li], 0), lx::MATCHES);
        for (int j = 0; j < R.lex_n[k]; j++) R.lex_matches[(size_t)k * lx::MATCHES + j] = P.lexm.h[(size_t)li * lx::MATCHES + j];
      }
    }
    if (P.pat.h) {   // rec patterns: a line without one reports pattern 0
      R.pat_id.assign((size_t)nb, 0); R.pat_res.assign((size_t)nb, pt::LineResult{0, 0.0f, 0.0f, 0.0f});
      const float* f = reinterpret_cast<const float*>(P.pat.h);
      for (int k = 0; k < nb; k++) {
        const int li = p.first_line + k;
        if (P.line_opts[li].pattern <= 0) continue;
        R.pat_id[k] = P.line_opts[li].pattern;
        R.pat_res[k] = pt::LineResult{P.pat.h[li] == 1 ? 1 : 0, f[P.NLp + li], f[2 * (size_t)P.NLp + li], f[3 * (size_t)P.NLp + li]};
      }
    }
    if (P.kwh.h) {   // rec keywords: a line without a list has 0 hits (its device slots were never written)
      R.kw_id.assign((size_t)nb, 0); R.kw_n.assign((size_t)nb, 0); R.kw_hits.assign((size_t)nb * kw::HITS, kw::Hit{});
      const double bw = P.crop_original ? (double)p.ori_w : (double)p.after_w, bh = P.crop_original ? (double)p.ori_h : (double)p.after_h;
      for (int k = 0; k < nb; k++) {
        const int li = p.first_line + k;
        if (P.line_opts[li].keywords <= 0) continue;
        R.kw_id[k] = P.line_opts[li].keywords;
        R.kw_n[k] = std::min(std::max(P.kwn.h[li], 0), kw::HITS);
        if (R.kw_n[k] == 0) continue;
        // the span [first_col, last_col + 1) as an ALNUM word's (wb::line_words): crop pixels per column, the crop's homography,
        // the line's rot180 as k_word_boxes takes it (the classifier's, inverted where rec flip took view 1), then
        // original-image coordinates
        const wb::WordGeom g = word_geom(P, li);
        const int rot180 = rf::rot180(m.label[li] == 1 && m.cscore[li] >= s.cfg.cls_thresh, P.flipo.h && P.both[(size_t)li] ? P.flipo.h[li] : rf::ONE_WAY);
        for (int j = 0; j < R.kw_n[k]; j++) {
          kw::Hit& h = R.kw_hits[(size_t)k * kw::HITS + j];
          h = P.kwh.h[(size_t)li * kw::HITS + j];
          kw::span_quad(h.first_col, h.last_col, g, rot180, h.quad);
          gm::scale_and_clip(h.quad, bw, bh, (double)p.ori_w, (double)p.ori_h);
        }
      }
    }
    if (P.bmn.h) {   // rec beams: per line its hypotheses, best first; a hypothesis' text from the dictionary as the line's own
      const int N = P.call.set.beam_n;
      R.beam_n = N; R.bm_count.assign((size_t)nb, 0); R.bm_recs.assign((size_t)nb * N, bm::Beam{0.0f, 0});
      R.bm_tokens.assign((size_t)nb * N, std::vector<int32_t>()); R.bm_text.assign((size_t)nb * N, std::string());
      if (P.bmlm.h) R.bm_lm.assign((size_t)nb * N, lm::BeamLm{0.0f, 0.0f});
      if (P.bmvc.h) R.bm_vocab.assign((size_t)nb * N, vc::BeamVocab{0, 0.0f});
      for (int k = 0; k < nb; k++) {
        const int li = p.first_line + k;
        const long long T = P.tok_off[li + 1] - P.tok_off[li];
        R.bm_count[k] = std::min(std::max(P.bmn.h[li], 0), N);
        for (int q = 0; q < R.bm_count[k]; q++) {
          bm::Beam& b = R.bm_recs[(size_t)k * N + q];
          b = P.bmrec.h[(size_t)li * N + q];
          b.n_tokens = (int32_t)std::min<long long>(std::max(b.n_tokens, 0), T);
          if (P.bmlm.h) R.bm_lm[(size_t)k * N + q] = P.bmlm.h[(size_t)li * N + q];
          if (P.bmvc.h) R.bm_vocab[(size_t)k * N + q] = P.bmvc.h[(size_t)li * N + q];
          const int* tk = P.bmtok.h + P.tok_off[li] * N + q * T;
          R.bm_tokens[(size_t)k * N + q].assign(tk, tk + b.n_tokens);
          std::string& t = R.bm_text[(size_t)k * N + q];
          for (int i = 0; i < b.n_tokens; i++) t += s.dict[(size_t)std::min<long long>(std::max(tk[i], 0), (long long)s.dict.size() - 1)];
        }
      }
    }
    if (s.cfg.rec_return_word_box) {   // word quads to original-image coordinates, word texts from the dictionary
      R.words.resize(nb); R.word_text.resize(nb);
      for (int k = 0; k < nb; k++) {
        const int li = p.first_line + k;
        const int nw = std::min(std::max(P.h_wcount[li], 0), m.ntok[li]);
        std::vector<wb::Word>& W = R.words[k];
        W.assign(P.h_words + P.tok_off[li], P.h_words + P.tok_off[li] + nw);
        R.word_text[k].resize((size_t)nw);
        // (crops planned on the original page: the homography already maps to original coordinates)
        const double bw = P.crop_original ? (double)p.ori_w : (double)p.after_w, bh = P.crop_original ? (double)p.ori_h : (double)p.after_h;
        for (int j = 0; j < nw; j++) {
          gm::scale_and_clip(W[j].quad, bw, bh, (double)p.ori_w, (double)p.ori_h);
          std::string& t = R.word_text[k][(size_t)j];
          for (int q = W[j].first_token; q < W[j].first_token + W[j].n_tokens; q++) t += s.dict[(size_t)R.tokens[k][(size_t)q]];
        }
      }
    }
  }
}
}  // namespace
std::string rt_format_f32_impl(float v) { return fnum(v); }

rt_results* rt_lane::run_pages(const PageCall& call) {
  const int n_pages = call.n_pages;
  if (g_trace) fprintf(stderr, "[rt host] %-28s %8.3f ms\n", "between calls", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - last_exit).count());
  HostTick tick0;
  // a one-page call is the reference's real mode (retto-cli/src/main.rs:80-86): it polls through its waits; a multi-page batch
  // is a throughput run whose lane threads must not hold a core each (8 ranks x 3 lanes on a 16-CPU pod)
  struct SpinScope { int& r; int old; ~SpinScope() { r = old; } } spin_scope{spin_us, spin_us};
  // (a lane worker's one-page part -- a batch of <= lanes pages, or several one-page submissions in flight -- is a throughput run
  //  too: it polls for a bounded 250 us per wait, not 5 ms)
  spin_us = n_pages > 1 ? 50 : call.on_lane_worker ? 250 : 5000;
  begin_call();
  tick0.lap("begin_call + arena reset");
  std::unique_ptr<rt_results> res(new rt_results());
  res->pages.resize((size_t)n_pages);
  if (n_pages == 0) return res.release();
  Pipeline P{call, std::vector<PageState>((size_t)n_pages)};
  P.crop_original = call.regions() || sh->cfg.crop_source == 1;
  HostTick tick;
  if (call.regions()) {   // the boxes are given: no resize_both, no detector, no DB post-processing, no first round trip
    region_pages(*this, P); tick.lap("pre (upload, regions)");
  } else {
    page_sizes(*this, P);
    tick.lap("pre (resize, upload)");
    det_groups(*this, P); tick.lap("det enqueue");
    db_post(*this, P); tick.lap("dbpost enqueue");
    box_round_trip(*this, P, *res); tick.lap("sync #1 + box D2H");
  }
  rt_refuse(expand_line_opts(P.pg.data(), n_pages, P.NL, call.regions() ? call.region_opts : nullptr, call.set.rec, sh->rec_counts(), P.line_opts, P.any));
  crop_stage(*this, P);
  if (P.NL > 0) {
    tick.lap("crop plan + warp enqueue");
    cls_stage(*this, P); tick.lap("cls enqueue");
    flip_plan(*this, P);   // (rec flip with 0 < cls_below <= 1: the call's one extra sync, for the classifier scores)
    rec_plan(*this, P);
    rec_groups(*this, P); tick.lap("rec enqueue");
    line_round_trip(*this, P);
  }
  tick.lap("sync #2 + D2H");
  results(*sh, P, *res);
  if (call.cb)
    for (int i = 0; i < n_pages; i++) { emit_stage(call, i, 1, res->pages[i]); emit_stage(call, i, 2, res->pages[i]); }
  tick.lap("results");
  if (g_trace) last_exit = std::chrono::steady_clock::now();
  return res.release();
}

// rt_debug_det_tiles: the det stage of a one-page call whose det image is the caller's -- det_groups itself, under the session's
// det tiles and det_sub_batch, so the launch groups are the pipeline's.  A page that is not tiled has one tile, its whole map.
void rt_session::debug_det_tiles(const uint8_t* rgb_det, int h, int w, float* tile_maps_out, float* page_map_out) {
  std::string why;
  const int rc = dt::check_page(h, w, &why);
  if (rc != dt::OK) throw RtError(rc, "rt_debug_det_tiles: " + why);
  begin_call();
  uint8_t* d = arena.alloc<uint8_t>((size_t)h * w * 3);
  RT_HIP_CHECK(hipMemcpyAsync(d, rgb_det, (size_t)h * w * 3, hipMemcpyHostToDevice, st));
  PageCall call;
  call.n_pages = 1; call.mem = RT_MEM_DEVICE; call.set = settings();
  Pipeline P{call, std::vector<PageState>(1)};
  PageState& p = P.pg[0];
  p.ori_h = p.after_h = p.det_h = h; p.ori_w = p.after_w = p.det_w = w;
  p.raw = p.img = p.det_img = d; p.map = nullptr;
  P.tile_maps_out = tile_maps_out;
  det_groups(*this, P);
  RT_HIP_CHECK(hipMemcpyAsync(page_map_out, p.map, (size_t)h * w * 4, hipMemcpyDeviceToHost, st));
  if (tile_maps_out && !dt::page_tiled(h, w, det_tile))
    RT_HIP_CHECK(hipMemcpyAsync(tile_maps_out, p.map, (size_t)h * w * 4, hipMemcpyDeviceToHost, st));
  sync();
}

// rt_debug_rec_windows: the lines as ONE rec group through rec_group_net, the function rec_groups runs per group, under the
// session's rec windows.  Without a windowed line the units are the lines.
void rt_session::debug_rec_windows(const float* nchw, int n, const int* widths, int32_t* unit_idx_out, float* unit_prob_out,
                                   float* unit_z5_out, int32_t* line_idx_out, float* line_prob_out, float* line_z5_out) {
  const int h = 48;
  size_t ne = 0, nt = 0;
  for (int i = 0; i < n; i++) {
    if (widths[i] < 8) throw RtError(RT_ERR_SHAPE, "rt_debug_rec_windows: every line must be at least 8 wide");
    ne += (size_t)3 * h * widths[i];
    nt += (size_t)RecNet::tokens_for_width(widths[i]);
  }
  begin_call();
  float* x = upload_ragged(*this, nchw, ne, n, h, widths);
  int* d_idx = arena.alloc<int>(nt); float* d_prob = arena.alloc<float>(nt);
  const float* z5 = nullptr;
  Level Lt;
  const RecWindowTaps taps{unit_idx_out, unit_prob_out, unit_z5_out};
  rec_group_net(*this, x, h, widths, n, rec_window, rec_overlap, d_idx, d_prob, &z5, Lt, &taps);
  if ((size_t)Lt.total != nt) throw RtError(RT_ERR_BACKEND, "rt_debug_rec_windows: token count mismatch");
  if (line_idx_out) RT_HIP_CHECK(hipMemcpyAsync(line_idx_out, d_idx, nt * 4, hipMemcpyDeviceToHost, st));
  if (line_prob_out) RT_HIP_CHECK(hipMemcpyAsync(line_prob_out, d_prob, nt * 4, hipMemcpyDeviceToHost, st));
  if (line_z5_out) RT_HIP_CHECK(hipMemcpyAsync(line_z5_out, z5, nt * rw::Z5_D * 4, hipMemcpyDeviceToHost, st));
  sync();
}

// rt_debug_rec_flip: the crops as ONE rec group through rec_group_flip, the function rec_groups runs for a group with a both-ways
// line (a call without one: the whole-line path of rec_groups, resize_norm and rec_group_net), under the session's rec windows.
void rt_session::debug_rec_flip(const uint8_t* crops, const int* hw, int n, const uint8_t* both, float max_wh_ratio, const RecFlipOut& out) {
  const int rh = cfg.rec_image_shape[1];
  const int W = gm::resize_norm_width(rh, cfg.rec_image_shape[2], max_wh_ratio);
  if (W < 8) throw RtError(RT_ERR_INVALID, "rt_debug_rec_flip: max_wh_ratio gives a line less than 8 wide");
  const int T = RecNet::tokens_for_width(W);
  size_t bytes = 0; int nf = 0;
  std::vector<pp::LineDesc> lines((size_t)n);
  std::vector<int> Ws((size_t)n, W);
  for (int i = 0; i < n; i++) {
    lines[(size_t)i] = line_desc(pp::CropRef{(long long)bytes, hw[2 * i], hw[2 * i + 1], 0}, hw[2 * i], hw[2 * i + 1], rh, W);
    bytes += (size_t)hw[2 * i] * hw[2 * i + 1] * 3;
    nf += both[i] ? 1 : 0;
  }
  begin_call();
  uint8_t* pool = arena.alloc<uint8_t>(bytes);
  RT_HIP_CHECK(hipMemcpyAsync(pool, crops, bytes, hipMemcpyHostToDevice, st));
  const size_t nt = (size_t)n * T;
  int* d_idx = arena.alloc<int>(std::max<size_t>(nt, 1)); float* d_prob = arena.alloc<float>(std::max<size_t>(nt, 1));
  int* d_out = arena.alloc<int>((size_t)n); float* d_sc = arena.alloc<float>((size_t)2 * n);
  RT_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)n * sizeof(int), st));
  const float* z5 = nullptr;
  Level Lt;
  const RecFlipTaps taps{out.view_idx, out.view_prob, out.view_z5, out.view_ntok, out.view_score};
  if (nf > 0) rec_group_flip(*this, pool, lines.data(), Ws.data(), both, n, 0, rh, rec_window, rec_overlap, d_idx, d_prob, &z5, Lt, d_out, d_sc, &taps);
  else {   // (no both-ways line: the group's former path, rec_groups' own steps; the views are the lines)
    pp::LineDesc* hl = pinned.alloc<pp::LineDesc>((size_t)n);
    for (int i = 0; i < n; i++) { hl[i] = lines[(size_t)i]; hl[i].out_off = (long long)i * rh * W * 4; }
    pp::LineDesc* dl = scratch.alloc<pp::LineDesc>((size_t)n);
    RT_HIP_CHECK(hipMemcpyAsync(dl, hl, (size_t)n * sizeof(pp::LineDesc), hipMemcpyHostToDevice, st));
    float* x = scratch.alloc<float>((size_t)n * rh * W * 4);
    pp::resize_norm(st, dl, n, rh, W, pool, 0, x, d_flags);
    rec_group_net(*this, x, rh, Ws.data(), n, rec_window, rec_overlap, d_idx, d_prob, &z5, Lt);
    int* v_tok = scratch.alloc<int>(std::max<size_t>(nt, 1)); int* v_ntok = scratch.alloc<int>((size_t)n); float* v_score = scratch.alloc<float>((size_t)n);
    pp::ctc_decode(st, d_idx, d_prob, Lt.d, n, v_tok, v_ntok, v_score);
    if (out.view_idx) RT_HIP_CHECK(hipMemcpyAsync(out.view_idx, d_idx, nt * 4, hipMemcpyDeviceToHost, st));
    if (out.view_prob) RT_HIP_CHECK(hipMemcpyAsync(out.view_prob, d_prob, nt * 4, hipMemcpyDeviceToHost, st));
    if (out.view_z5) RT_HIP_CHECK(hipMemcpyAsync(out.view_z5, z5, nt * rw::Z5_D * 4, hipMemcpyDeviceToHost, st));
    if (out.view_ntok) RT_HIP_CHECK(hipMemcpyAsync(out.view_ntok, v_ntok, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (out.view_score) RT_HIP_CHECK(hipMemcpyAsync(out.view_score, v_score, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  }
  if ((size_t)Lt.total != nt) throw RtError(RT_ERR_BACKEND, "rt_debug_rec_flip: token count mismatch");
  std::vector<int> h_out((size_t)n);
  RT_HIP_CHECK(hipMemcpyAsync(h_out.data(), d_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  if (out.idx) RT_HIP_CHECK(hipMemcpyAsync(out.idx, d_idx, nt * 4, hipMemcpyDeviceToHost, st));
  if (out.prob) RT_HIP_CHECK(hipMemcpyAsync(out.prob, d_prob, nt * 4, hipMemcpyDeviceToHost, st));
  if (out.z5) RT_HIP_CHECK(hipMemcpyAsync(out.z5, z5, nt * rw::Z5_D * 4, hipMemcpyDeviceToHost, st));
  sync(); check_flags();
  if (out.taken) for (int i = 0; i < n; i++) out.taken[i] = h_out[(size_t)i] == rf::TOOK_1 ? 1 : 0;
}

const char* rt_results_json_impl(rt_results* r, int page, int stage) {
  rt_results::Page& P = r->pages[(size_t)page];
  P.json[stage] = stage_json(P, stage);
  return P.json[stage].c_str();
}

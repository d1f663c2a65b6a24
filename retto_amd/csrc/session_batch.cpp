// The session's lanes at work: the lanes' host threads, tickets (rt_submit_batch / rt_wait_batch), page staging, encoded pages
// (rt_submit_encoded_batch, rt_decode_batch), and the entry points that split a call over the lanes (rt_run_batch,
// rt_run_regions*).  What a lane runs is rt_lane::run_pages (session.cpp); how the pages are split is lane_split.h.
#include "session.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "geom_math.h"

using namespace rt;

// ---------------------------------------------------------------------------
// Lanes.  A batch's pages are split over the lanes (contiguous ranges, order preserved); every lane is a full pipeline on its own
// stream, so one lane's small kernels, launch gaps and host sync points overlap the other lanes' large kernels.  The lanes' host
// threads are persistent, and batches can be SUBMITTED ahead (rt_submit_batch / rt_wait_batch, the counterpart of
// RettoSession::run_stream's worker thread + channel, session.rs:108-143): a lane that has finished its part of batch i starts
// on batch i + 1 at once, so the lanes drift apart in phase and the call boundary (result assembly on the host, descriptors of
// the next call) no longer idles the GPU.
// ---------------------------------------------------------------------------
void LaneWorker::start(int device) {
  th = std::thread([this, device] {
    (void)hipSetDevice(device);
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !q.empty(); });
        if (q.empty()) return;   // stop requested and nothing left
        f = std::move(q.front()); q.pop_front();
      }
      f();
    }
  });
}
void LaneWorker::push(std::function<void()> f) {
  { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(f)); }
  cv.notify_one();
}
void LaneWorker::shutdown() {
  { std::lock_guard<std::mutex> lk(mu); stop = true; }
  cv.notify_all();
  if (th.joinable()) th.join();
}
void rt_session::ensure_workers() {
  while ((int)workers.size() < n_lanes()) {
    std::unique_ptr<LaneWorker> w(new LaneWorker());
    w->start(device);
    workers.push_back(std::move(w));
  }
}

// ---- page staging ----------------------------------------------------------------------------------------------------------
// A lane that uploads its own pages blocks its host thread in hipMemcpyAsync (pageable memory: the call returns when the copy is
// done) with nothing queued on its stream: about 3 ms per 11-page part.  rt_submit_batch therefore copies the host pages of the
// whole batch itself, on a copy stream, into a slot of HBM the session keeps per batch in flight; the lanes' streams wait for the
// slot's event.  With one batch submitted ahead the copy of batch i+1 runs on the DMA engines under the kernels of batch i.
int rt_session::acquire_slot(size_t total, int nl) {
  RT_HIP_CHECK(hipSetDevice(device));   // (the caller's thread: nothing else has chosen the device on the submit path)
  int slot = -1;
  for (size_t k = 0; k < stage_slots.size(); k++) if (!stage_slots[k].busy) { slot = (int)k; break; }
  if (slot < 0) { stage_slots.emplace_back(); slot = (int)stage_slots.size() - 1; }
  StageSlot& S = stage_slots[(size_t)slot];
  if (!st_copy) RT_HIP_CHECK(hipStreamCreateWithFlags(&st_copy, hipStreamNonBlocking));
  while ((int)S.ev.size() < nl) {
    hipEvent_t e = nullptr;
    RT_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    S.ev.push_back(e);
  }
  if (S.cap < total) {
    if (S.p) { (void)hipFree(S.p); S.p = nullptr; S.cap = 0; }
    if (hipMalloc((void**)&S.p, total) != hipSuccess) { (void)hipGetLastError(); S.p = nullptr; return -1; }
    S.cap = total;
  }
  return slot;
}

// ---- encoded pages (rt_submit_encoded_batch, rt_decode_batch) -----------------------------------------------------------------
// Layout of pages [i0, i1) inside a slot from byte `at`: each page's RGB8 result, then for a page the kernels reconstruct its
// MCU-padded component planes and int16 coefficients, then the part's DevComp / DevPage tables.  Returns the end offset.
static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t enc_layout(const std::vector<rt::EncodedPage>& enc, int i0, int i1, size_t at, std::vector<size_t>& rgb_off,
                         rt_ticket::EncPart& P) {
  int64_t blocks = 0;
  for (int i = i0; i < i1; i++) {
    const rt::EncodedPage& e = enc[(size_t)i];
    rgb_off[(size_t)i] = at;
    at += al256((size_t)e.h * e.w * 3);
    if (!e.on_device) continue;
    const rt::JpegCoefs& J = e.jpeg;
    rt::jpeg::DevPage dp{};
    dp.rgb_off = rgb_off[(size_t)i]; dp.pix_base = P.pixels; dp.W = J.W; dp.H = J.H; dp.nc = J.nc; dp.is_rgb = J.is_rgb;
    for (int k = 0; k < J.nc; k++) {
      const rt::JpegCoefs::Comp& C = J.c[k];
      rt::jpeg::DevComp dc{};
      dc.plane_off = at; at += al256((size_t)C.stride * C.rows);
      dc.coef_off = at; at += al256(C.coef.size() * sizeof(int16_t));
      dc.blocks_w = C.stride / 8; dc.nblocks = (C.stride / 8) * (C.rows / 8); dc.block_base = (int)blocks;
      blocks += dc.nblocks;
      if (blocks > 0x7fffffff || C.coef.size() != (size_t)dc.nblocks * 64) throw RtError(RT_ERR_BACKEND, "encoded batch: too many JPEG blocks in one part");
      dc.stride = C.stride; dc.cw = C.cw; dc.ch = C.ch; dc.fh = J.hmax / C.hs; dc.fv = J.vmax / C.vs;
      memcpy(dc.q, C.q, sizeof(dc.q));
      dp.comp[k] = (int)P.comps.size();
      P.comps.push_back(dc);
    }
    P.pixels += (int64_t)J.W * J.H;
    P.pages.push_back(dp);
  }
  P.blocks = (int)blocks;
  P.comps_off = at; at += al256(P.comps.size() * sizeof(rt::jpeg::DevComp));
  P.pages_off = at; at += al256(P.pages.size() * sizeof(rt::jpeg::DevPage));
  return at;
}
// uploads pages [i0, i1) (coefficients of the device pages, pixels of the others) and the tables, then reconstructs on `st`
static void enc_upload(uint8_t* base, const std::vector<rt::EncodedPage>& enc, int i0, int i1, const std::vector<size_t>& rgb_off,
                       const rt_ticket::EncPart& P, hipStream_t st) {
  size_t c = 0;
  for (int i = i0; i < i1; i++) {
    const rt::EncodedPage& e = enc[(size_t)i];
    if (!e.on_device) {
      RT_HIP_CHECK(hipMemcpyAsync(base + rgb_off[(size_t)i], e.rgb.data(), e.rgb.size(), hipMemcpyHostToDevice, st));
      continue;
    }
    for (int k = 0; k < e.jpeg.nc; k++, c++) {
      const std::vector<int16_t>& q = e.jpeg.c[k].coef;
      RT_HIP_CHECK(hipMemcpyAsync(base + P.comps[c].coef_off, q.data(), q.size() * sizeof(int16_t), hipMemcpyHostToDevice, st));
    }
  }
  if (P.pages.empty()) return;
  RT_HIP_CHECK(hipMemcpyAsync(base + P.comps_off, P.comps.data(), P.comps.size() * sizeof(rt::jpeg::DevComp), hipMemcpyHostToDevice, st));
  RT_HIP_CHECK(hipMemcpyAsync(base + P.pages_off, P.pages.data(), P.pages.size() * sizeof(rt::jpeg::DevPage), hipMemcpyHostToDevice, st));
  const auto* comps = (const rt::jpeg::DevComp*)(base + P.comps_off);
  rt::launch_jpeg_idct(base, comps, (int)P.comps.size(), P.blocks, st);
  rt::launch_jpeg_color(base, comps, (const rt::jpeg::DevPage*)(base + P.pages_off), (int)P.pages.size(), P.pixels, st);
}
// an encoded ticket: every part in one slot, laid out part after part (staging is not optional here: the lanes need pixels)
static void stage_encoded_layout(rt_ticket* t, size_t* total) {
  t->enc_parts.assign((size_t)t->nl, rt_ticket::EncPart());
  t->stage_off.assign((size_t)t->call.n_pages, (size_t)-1);
  size_t at = 0;
  for (int l = 0; l < t->nl; l++) at = enc_layout(t->enc, t->first[l], t->first[l + 1], at, t->stage_off, t->enc_parts[(size_t)l]);
  *total = at;
}
void rt_session::decode_batch(std::vector<rt::EncodedPage>& enc, uint8_t* const* out, int mem) {
  const int n = (int)enc.size();
  std::vector<size_t> off((size_t)n, 0);
  rt_ticket::EncPart P;
  const size_t total = enc_layout(enc, 0, n, 0, off, P);
  bool any_dev = false;
  for (auto& e : enc) any_dev |= e.on_device || mem == RT_MEM_DEVICE;
  if (!any_dev) {   // host pages into host memory: nothing to do on the device
    for (int i = 0; i < n; i++) memcpy(out[i], enc[(size_t)i].rgb.data(), enc[(size_t)i].rgb.size());
    return;
  }
  const int slot = acquire_slot(std::max<size_t>(total, 256), 1);
  if (slot < 0) throw RtError(RT_ERR_BACKEND, "rt_decode_batch: out of device memory for the pages");
  uint8_t* base = stage_slots[(size_t)slot].p;
  enc_upload(base, enc, 0, n, off, P, st_copy);
  for (int i = 0; i < n; i++) {
    const rt::EncodedPage& e = enc[(size_t)i];
    const size_t bytes = (size_t)e.h * e.w * 3;
    if (mem == RT_MEM_DEVICE) RT_HIP_CHECK(hipMemcpyAsync(out[i], base + off[(size_t)i], bytes, hipMemcpyDeviceToDevice, st_copy));
    else if (e.on_device) RT_HIP_CHECK(hipMemcpyAsync(out[i], base + off[(size_t)i], bytes, hipMemcpyDeviceToHost, st_copy));
    else memcpy(out[i], e.rgb.data(), bytes);
  }
  RT_HIP_CHECK(hipStreamSynchronize(st_copy));
}

void rt_session::stage_pages(rt_ticket* t) {
  if (!t->enc.empty()) {
    size_t total = 0;
    stage_encoded_layout(t, &total);
    const int slot = acquire_slot(std::max<size_t>(total, 256), t->nl);
    if (slot < 0) throw RtError(RT_ERR_BACKEND, "rt_submit_encoded_batch: out of device memory for the pages");
    StageSlot& S = stage_slots[(size_t)slot];
    S.busy = true;
    t->stage_slot = slot;
    t->ev_up.assign(S.ev.begin(), S.ev.begin() + t->nl);
    for (int i = 0; i < t->call.n_pages; i++) t->rgb[(size_t)i] = S.p + t->stage_off[(size_t)i];
    t->call.mem = RT_MEM_STAGED_MAPS_HOST;
    return;
  }
  if (t->call.mem != RT_MEM_HOST && t->call.mem != RT_MEM_HOST_MAPS_DEVICE) return;
  size_t total = 0;
  std::vector<size_t> off((size_t)t->call.n_pages, (size_t)-1);
  for (int i = 0; i < t->call.n_pages; i++) {
    if (t->hs[i] <= 0 || t->ws[i] <= 0 || !t->rgb[i]) continue;   // left to the lane, which reports it as the reference does
    off[(size_t)i] = total;
    total += ((size_t)t->hs[i] * t->ws[i] * 3 + 255) & ~(size_t)255;
  }
  if (!total) return;
  const int slot = acquire_slot(total, t->nl);
  if (slot < 0) return;   // out of device memory: the lanes copy, as before
  StageSlot& S = stage_slots[(size_t)slot];
  S.busy = true;
  t->stage_slot = slot;
  t->stage_off = std::move(off);
  t->ev_up.assign(S.ev.begin(), S.ev.begin() + t->nl);
  t->call.mem = t->call.mem == RT_MEM_HOST ? RT_MEM_STAGED_MAPS_HOST : RT_MEM_DEVICE;
}
// the part's pages go up right before its lane job is queued: the first lane starts after its own pages, not after the batch's
void rt_session::stage_part(rt_ticket* t, int l) {
  if (t->stage_slot < 0) return;
  StageSlot& S = stage_slots[(size_t)t->stage_slot];
  if (!t->enc.empty()) {
    enc_upload(S.p, t->enc, t->first[l], t->first[l + 1], t->stage_off, t->enc_parts[(size_t)l], st_copy);
    RT_HIP_CHECK(hipEventRecord(t->ev_up[(size_t)l], st_copy));
    return;
  }
  for (int i = t->first[l]; i < t->first[l + 1]; i++) {
    const size_t o = t->stage_off[(size_t)i];
    if (o == (size_t)-1) continue;
    RT_HIP_CHECK(hipMemcpyAsync(S.p + o, t->rgb[i], (size_t)t->hs[i] * t->ws[i] * 3, hipMemcpyHostToDevice, st_copy));
    t->rgb[i] = S.p + o;
  }
  RT_HIP_CHECK(hipEventRecord(t->ev_up[(size_t)l], st_copy));
}
void rt_session::release_stage(rt_ticket* t) {
  if (t->stage_slot >= 0) stage_slots[(size_t)t->stage_slot].busy = false;
  t->stage_slot = -1;
}
void rt_session::free_stage() {
  if (st_copy) (void)hipStreamSynchronize(st_copy);
  for (auto& S : stage_slots) { if (S.p) (void)hipFree(S.p); for (hipEvent_t e : S.ev) (void)hipEventDestroy(e); }
  stage_slots.clear();
  if (st_copy) { (void)hipStreamDestroy(st_copy); st_copy = nullptr; }
}

rt_ticket* rt_session::submit_batch(const PageCall& call, std::vector<rt::EncodedPage>* enc) {
  if (!call.regions()) rt_refuse(rec_opts_conflict(rec_default));   // (regions: run_regions has checked every region's own options)
  ensure_workers();
  std::unique_ptr<rt_ticket> t(new rt_ticket());
  const int n_pages = call.n_pages, nl = lanes_for(n_pages);
  t->nl = nl;
  t->rgb.assign(call.rgb, call.rgb + n_pages); t->hs.assign(call.hs, call.hs + n_pages); t->ws.assign(call.ws, call.ws + n_pages);
  if (call.det_map_override) t->maps.assign(call.det_map_override, call.det_map_override + n_pages);
  // (the lanes run later: the call is the submitting one's, settings included, over the ticket's copies of its arrays)
  t->call = call;
  t->call.rgb = t->rgb.data(); t->call.hs = t->hs.data(); t->call.ws = t->ws.data();
  t->call.det_map_override = t->maps.empty() ? nullptr : t->maps.data();
  t->call.cb_mu = &t->cb_mu; t->call.page_base = 0; t->call.on_lane_worker = true;
  t->parts.assign((size_t)nl, nullptr); t->errs.resize((size_t)nl);
  t->first = lane_split(call.hs, call.ws, n_pages, cfg.max_side_len, nl);
  t->remaining = nl;
  rt_ticket* tp = t.get();
  static const bool no_stage = getenv("RT_NO_STAGE") && atoi(getenv("RT_NO_STAGE"));   // (A/B switch of the measurement in DESIGN.md)
  if (enc) tp->enc = std::move(*enc);
  if (!no_stage || !tp->enc.empty()) stage_pages(tp);
  // parts go to consecutive lanes starting behind the previous batch's last one: batches that fill fewer lanes than the session
  // has (single pages: one lane each) run side by side instead of queueing on lane 0
  const int total_lanes = n_lanes();
  // (with rt_set_lanes below the session's lane count the partitions would leave CUs unused: whole-device streams then)
  const bool use_parts = active_lanes >= total_lanes;
  const int base = next_lane;
  next_lane = (next_lane + nl) % total_lanes;
  int queued = 0;
  try {
  for (int l = 0; l < nl; l++) {
    const int li = (base + l) % total_lanes;
    rt_lane* s = lane(li);
    stage_part(tp, l);
    workers[(size_t)li]->push([tp, s, l, use_parts] {
      const PageCall part = tp->call.part(tp->first[l], tp->first[l + 1]);
      // a lane inside a submitted batch works on its own CU partition (every call ends with its stream drained, so the lane's
      // arenas and pinned staging can change streams between calls)
      s->st = (s->st_part && use_parts) ? s->st_part : s->st_full;
      try {
        if (!tp->ev_up.empty()) RT_HIP_CHECK(hipStreamWaitEvent(s->st, tp->ev_up[(size_t)l], 0));
        tp->parts[l] = s->run_pages(part);
      } catch (...) {
        tp->errs[l] = std::current_exception();
        s->failed = true;
        // work of the failed part may still be queued on the lane's stream: drain it before the lane's next job rewinds the
        // arenas and the pinned staging it reads
        if (s->st) (void)hipStreamSynchronize(s->st);
        (void)hipGetLastError();
      }
      s->st = s->st_full;
      // notify while holding the mutex: rt_wait_batch owns the ticket and deletes it as soon as it sees remaining == 0, so
      // nothing of *tp may be touched once the decrement is visible outside the lock
      { std::lock_guard<std::mutex> lk(tp->mu); tp->remaining--; tp->cv.notify_all(); }
    });
    queued++;
  }
  } catch (...) {
    // a push that threw (bad_alloc): the parts already queued hold tp -- take the un-queued ones off the count, wait for the
    // queued ones, and leave the session as it was (inflight is only counted once every part is queued)
    {
      std::unique_lock<std::mutex> lk(tp->mu);
      tp->remaining -= nl - queued;
      tp->cv.wait(lk, [&] { return tp->remaining == 0; });
    }
    for (auto* r : tp->parts) delete r;
    release_stage(tp);
    throw;
  }
  inflight.fetch_add(1);
  return t.release();
}

rt_results* rt_session::wait_batch(rt_ticket* tp) {
  std::unique_ptr<rt_ticket> t(tp);
  {
    std::unique_lock<std::mutex> lk(t->mu);
    t->cv.wait(lk, [&] { return t->remaining == 0; });
  }
  inflight.fetch_sub(1);
  release_stage(t.get());   // (every lane has drained its stream: nothing reads the slot any more)
  std::unique_ptr<rt_results> res(new rt_results());
  std::exception_ptr err;
  for (int l = 0; l < t->nl; l++) {
    if (t->errs[l] && !err) err = t->errs[l];
    if (t->parts[l]) {
      for (auto& p : t->parts[l]->pages) res->pages.push_back(std::move(p));
      res->det_checksum += t->parts[l]->det_checksum;
      delete t->parts[l];
    }
  }
  if (err) std::rethrow_exception(err);
  return res.release();
}

// a call that takes one lane: on the caller's thread (no hand-over in the single-page latency path)
rt_results* rt_session::run_on_caller(const PageCall& call) {
  try {
    return run_pages(call);
  } catch (...) { failed = true; throw; }
}

rt_results* rt_session::run_batch(const PageCall& call) {
  if (lanes_for(call.n_pages) > 1) return wait_batch(submit_batch(call));
  rt_refuse(rec_opts_conflict(rec_default));
  return run_on_caller(call);
}

// rt_run_regions.  A quad is clamped to the page, then held to what the crop plan needs: a crop of at least 1 x 1 pixels and an
// invertible homography -- checked here, for every page, before anything is queued.
rt_results* rt_session::run_regions(const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                                    const float* const* quads, const int* n_quads, const int* const* const ids[REC_N_KINDS]) {
  std::vector<std::vector<float>> clamped((size_t)n_pages);
  std::vector<const float*> qp((size_t)n_pages, nullptr);
  // the regions' options with -1 resolved to the session defaults of this call (rec_line_opts.h)
  std::vector<std::vector<RecLineOpts>> opts((size_t)n_pages);
  std::vector<const RecLineOpts*> op((size_t)n_pages, nullptr);
  for (int i = 0; i < n_pages; i++) {
    const std::string where = "rt_run_regions: page " + std::to_string(i);
    if (hs[i] <= 0 || ws[i] <= 0 || rgb[i] == nullptr) throw RtError(RT_ERR_IMAGE, where + ": empty page");
    if (n_quads[i] < 0) throw RtError(RT_ERR_INVALID, where + ": negative region count");
    if (n_quads[i] > 0 && quads[i] == nullptr) throw RtError(RT_ERR_INVALID, where + ": NULL quads with a positive region count");
    std::vector<float>& q = clamped[(size_t)i];
    q.resize((size_t)n_quads[i] * 8);
    const float mx = (float)(ws[i] - 1), my = (float)(hs[i] - 1);
    for (int k = 0; k < n_quads[i]; k++) {
      const std::string at = where + " region " + std::to_string(k);
      float* b = q.data() + 8 * (size_t)k;
      for (int j = 0; j < 8; j++) {
        const float v = quads[i][8 * (size_t)k + j], hi = (j & 1) ? my : mx;
        if (!std::isfinite(v)) throw RtError(RT_ERR_INVALID, at + ": non-finite coordinate");
        b[j] = v < 0.0f ? 0.0f : (v > hi ? hi : v);
      }
      const gm::CropDims d = gm::crop_dims(b);
      if (d.w < 1 || d.h < 1) throw RtError(RT_ERR_INVALID, at + ": the crop is smaller than one pixel");
      float inv[9];
      if (!gm::projection_inverse(b, d.cw, d.ch, inv)) throw RtError(RT_ERR_INVALID, at + ": singular homography (degenerate quad)");
    }
    qp[(size_t)i] = q.data();
    // (a page's options behind the checks of its quads and before the next page's)
    const std::string bad = resolve_region_opts(i, i + 1, n_quads, ids, REC_N_KINDS, rec_default, rec_counts(), opts);
    if (!bad.empty()) throw RtError(RT_ERR_INVALID, "rt_run_regions: " + bad);
    op[(size_t)i] = opts[(size_t)i].data();
  }
  PageCall call = call_of(rgb, hs, ws, n_pages, mem);
  call.quads = qp.data(); call.n_quads = n_quads; call.region_opts = op.data();
  // (more than one lane: clamped and opts outlive the wait)
  return lanes_for(n_pages) > 1 ? wait_batch(submit_batch(call)) : run_on_caller(call);
}

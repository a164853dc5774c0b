// rnamc_entries_window.cpp — rnamc_window_plan and rnamc_bpp_windowed: the windows of one long
// sequence through the bpp sweep chunk by chunk and group by group, and per group the integer
// accumulation of its device-resident triangles into the band of the whole sequence
// (rnamc_window.hip).
#include "rnamc_entries.h"

using namespace rnamc;

namespace rnamc {

int window_plan_of(uint64_t n, uint32_t window, uint32_t stride, uint32_t max_bp_span, WindowPlan* out) {
  if (window == 0 || stride == 0 || window > RNAMC_MAX_SEQ_LEN) {
    set_last_error("rnamc_bpp_windowed: window must be 1 .. 65535 and stride >= 1");
    return RNAMC_ERR_INVALID_ARG;
  }
  if (n == 0) return RNAMC_ERR_EMPTY_SEQ;
  if (n >= (1ull << 31)) {
    set_last_error("rnamc_bpp_windowed: n must be below 2^31");
    return RNAMC_ERR_INVALID_ARG;
  }
  WindowPlan wp;
  wp.n = n;
  wp.stride = stride;
  wp.w = static_cast<uint32_t>(std::min<uint64_t>(window, n));
  wp.n_grid = (n - wp.w) / stride + 1;  // starts x * stride with x * stride + w <= n
  wp.has_last = (wp.n_grid - 1) * stride + wp.w < n ? 1u : 0u;
  wp.n_windows = wp.n_grid + wp.has_last;
  wp.band = wp.w;
  if (max_bp_span != 0) wp.band = std::min(wp.band, max_bp_span);
  *out = wp;
  return RNAMC_OK;
}

int bpp_windowed_check(const uint8_t* bases, uint64_t n, const char* constraint, uint32_t window, uint32_t stride,
                       uint32_t max_bp_span, const float* band_prob, WindowPlan* out) {
  if (!bases || !band_prob) return RNAMC_ERR_INVALID_ARG;
  if (int rc = window_plan_of(n, window, stride, max_bp_span, out)) return rc;
  for (uint64_t x = 0; x < n; x++)
    if (bases[x] > 3) return RNAMC_ERR_INVALID_BASE;
  if (constraint)
    for (uint64_t x = 0; x < n; x++) {
      const char ch = constraint[x];
      if (ch == '.' || ch == 'x' || ch == '<' || ch == '>') continue;
      set_last_error("rnamc_bpp_windowed: constraint position " + std::to_string(x) +
                     ((ch == '(' || ch == ')') ? ": brackets cannot be cut at window edges (only . x < > are allowed)"
                                               : ": byte outside . x < >"));
      return RNAMC_ERR_INVALID_ARG;
    }
  return RNAMC_OK;
}

namespace {

WindowGeom geom_of(const WindowPlan& wp) {
  WindowGeom g{};
  g.n = wp.n;
  g.n_grid = wp.n_grid;
  g.w = wp.w;
  g.stride = wp.stride;
  g.band = wp.band;
  g.has_last = wp.has_last;
  return g;
}

}  // namespace

int bpp_windowed_accumulate(rnamc_ctx* c, const WindowPlan& wp, const uint8_t* bases, const char* constraint,
                            uint64_t first, uint64_t count, int uses_contra_model, int allows_short_hairpins,
                            float* window_log_partition) {
  hipStream_t st = c->own_stream;  // (a call with hooks never takes the two-stream route of the tree order)
  const uint64_t cells = static_cast<uint64_t>(wp.band) * wp.n;
  const uint32_t w = wp.w;
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(c->wn_sum.grow(cells));
  HIPCHK(c->wn_cnt.grow(cells));
  // once per call, not per chunk
  HIPCHK(hipMemsetAsync(c->wn_sum, 0, cells * sizeof(int64_t), st));
  HIPCHK(hipMemsetAsync(c->wn_cnt, 0, cells * sizeof(uint32_t), st));
  rnamc_batch_stats total{};
  if (count == 0) {
    c->stats = total;
    return RNAMC_OK;
  }
  ChunkScan s{};
  s.who = "rnamc_bpp_windowed";
  s.what = "windows";
  s.rec_len = w;
  s.count = count;
  // windows of a chunk: window_chunk_nt nucleotides, one window at least, a u32 of records at most
  s.per_chunk = std::min<uint64_t>(
      std::min<uint64_t>(std::max<uint64_t>(static_cast<uint64_t>(c->window_chunk_nt) / w, 1), count), 0xffffffffull);
  s.with_constraint = constraint != nullptr;
  s.max_bp_span = wp.band;
  s.contra = uses_contra_model != 0;
  s.allows_short = allows_short_hairpins != 0;
  s.log_partition = window_log_partition ? window_log_partition + first : nullptr;
  s.events = &c->wn_events;
  s.launches_own = &rnamc_batch_stats::launches_window;
  s.ms_own = &rnamc_batch_stats::ms_window;
  std::vector<WindowItem> items;  // (the host copy lives until the chunk's stream is drained)
  try {  // nothing may throw across the C boundary
    items.resize(s.per_chunk);
  } catch (const std::exception&) {
    set_last_error("rnamc_bpp_windowed: no host memory for a chunk of windows");
    return RNAMC_ERR_OOM;
  }
  s.cut = [&](uint64_t x, uint8_t* rec, char* cons) {
    const uint64_t at = wp.start(first + x);
    std::memcpy(rec, bases + at, w);
    if (cons) std::memcpy(cons, constraint + at, w);
  };
  s.upload_items = [&](uint64_t x0, uint32_t m) -> int {
    for (size_t x = 0; x < c->descs.size(); x++) {
      const SeqDesc& sd = c->descs[x];
      items[x].bpp_off = sd.out_off;
      items[x].start = wp.start(first + x0 + sd.batch_idx);
    }
    HIPCHK(c->wn_items.upload(items.data(), m, st));
    return RNAMC_OK;
  };
  s.launch = [&](uint32_t first_desc, uint32_t k) -> uint64_t {
    launch_window_accumulate(c->wn_items + first_desc, k, c->st_out[0], w, wp.band, wp.n, c->wn_sum, c->wn_cnt, st);
    return 1;
  };
  if (int rc = scan_chunks(c, s, &total)) return rc;
  c->stats = total;
  return RNAMC_OK;
}

int bpp_windowed_fetch(rnamc_ctx* c, const WindowPlan& wp, int64_t* sum, uint32_t* cnt) {
  const uint64_t cells = static_cast<uint64_t>(wp.band) * wp.n;
  HIPCHK(hipMemcpyAsync(sum, c->wn_sum, cells * sizeof(int64_t), hipMemcpyDeviceToHost, c->own_stream));
  HIPCHK(hipMemcpyAsync(cnt, c->wn_cnt, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->own_stream));
  HIPCHK(hipStreamSynchronize(c->own_stream));
  return RNAMC_OK;
}

int bpp_windowed_finish(rnamc_ctx* c, const WindowPlan& wp, const int64_t* sum, const uint32_t* cnt,
                        float* band_prob, float* paired_prob) {
  hipStream_t st = c->own_stream;
  const uint64_t cells = static_cast<uint64_t>(wp.band) * wp.n;
  if (sum) {  // the totals of a pool's shards
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(c->wn_sum.grow(cells));
    HIPCHK(c->wn_cnt.grow(cells));
    HIPCHK(hipMemcpyAsync(c->wn_sum, sum, cells * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->wn_cnt, cnt, cells * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  HIPCHK(c->wn_band.grow(cells));
  if (paired_prob) HIPCHK(c->wn_paired.grow(wp.n));
  const bool prof = c->profile != 0;
  if (prof) {
    HIPCHK(c->wn_events.pairs(1));
    HIPCHK(hipEventRecord(c->wn_events[0], st));
  }
  const WindowGeom g = geom_of(wp);
  launch_window_finalize(g, c->wn_sum, c->wn_cnt, c->wn_band, st);
  uint64_t launches = 1;
  if (paired_prob) {
    launch_window_paired(g, c->wn_sum, c->wn_cnt, c->wn_paired, st);
    launches++;
  }
  HIPCHK(hipGetLastError());
  if (prof) HIPCHK(hipEventRecord(c->wn_events[1], st));
  HIPCHK(hipMemcpyAsync(band_prob, c->wn_band, cells * sizeof(float), hipMemcpyDeviceToHost, st));
  if (paired_prob)
    HIPCHK(hipMemcpyAsync(paired_prob, c->wn_paired, wp.n * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->stats.launches_other += launches;
  c->stats.launches_window += launches;
  if (prof) HIPCHK(c->wn_events.pairs_ms(1, &c->stats.ms_window));
  return RNAMC_OK;
}

}  // namespace rnamc

extern "C" {

int rnamc_window_plan(uint64_t n, uint32_t window, uint32_t stride, uint32_t max_bp_span, uint64_t* n_windows,
                      uint32_t* band, uint64_t* starts, uint64_t starts_cap) {
  if (!n_windows) return RNAMC_ERR_INVALID_ARG;
  WindowPlan wp;
  if (int rc = window_plan_of(n, window, stride, max_bp_span, &wp)) return rc;
  *n_windows = wp.n_windows;
  if (band) *band = wp.band;
  if (!starts) return RNAMC_OK;
  if (starts_cap < wp.n_windows) {
    set_last_error("rnamc_window_plan: " + std::to_string(wp.n_windows) + " windows, starts_cap " +
                   std::to_string(starts_cap));
    return RNAMC_ERR_INVALID_ARG;
  }
  for (uint64_t x = 0; x < wp.n_windows; x++) starts[x] = wp.start(x);
  return RNAMC_OK;
}

int rnamc_bpp_windowed(rnamc_ctx* c, const uint8_t* bases, uint64_t n, const char* constraint, uint32_t window,
                       uint32_t stride, uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                       float* band_prob, float* paired_prob, float* window_log_partition) {
  if (!c) return RNAMC_ERR_INVALID_ARG;
  WindowPlan wp;
  if (int rc = bpp_windowed_check(bases, n, constraint, window, stride, max_bp_span, band_prob, &wp)) return rc;
  std::unique_lock<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  if (int rc = bpp_windowed_accumulate(c, wp, bases, constraint, 0, wp.n_windows, uses_contra_model,
                                       allows_short_hairpins, window_log_partition)) {
    (void)hipStreamSynchronize(c->own_stream);
    return rc;
  }
  return bpp_windowed_finish(c, wp, nullptr, nullptr, band_prob, paired_prob);
}

}  // extern "C"

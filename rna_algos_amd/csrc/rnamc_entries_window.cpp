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
  HIPCHK(grow_device(reinterpret_cast<void**>(&c->wn_sum), &c->wn_sum_cap, cells * sizeof(int64_t)));
  HIPCHK(grow_device(reinterpret_cast<void**>(&c->wn_cnt), &c->wn_cnt_cap, cells * sizeof(uint32_t)));
  // once per call, not per chunk
  HIPCHK(hipMemsetAsync(c->wn_sum, 0, cells * sizeof(int64_t), st));
  HIPCHK(hipMemsetAsync(c->wn_cnt, 0, cells * sizeof(uint32_t), st));
  rnamc_batch_stats total{};
  if (count == 0) {
    c->stats = total;
    return RNAMC_OK;
  }
  // windows of a chunk: window_chunk_nt nucleotides, one window at least, a u32 of records at most
  const uint64_t per_chunk = std::min<uint64_t>(
      std::min<uint64_t>(std::max<uint64_t>(static_cast<uint64_t>(c->window_chunk_nt) / w, 1), count), 0xffffffffull);
  std::vector<uint8_t> cb;
  std::vector<char> cc;
  std::vector<uint64_t> offs;
  std::vector<WindowItem> items;
  try {  // nothing may throw across the C boundary
    cb.resize(per_chunk * w);
    if (constraint) cc.resize(per_chunk * w);
    offs.resize(per_chunk + 1);
    items.resize(per_chunk);
  } catch (const std::exception&) {
    set_last_error("rnamc_bpp_windowed: no host memory for a chunk of windows");
    return RNAMC_ERR_OOM;
  }
  const bool prof = c->profile != 0;
  for (uint64_t x0 = 0; x0 < count; x0 += per_chunk) {
    const uint32_t m = static_cast<uint32_t>(std::min<uint64_t>(per_chunk, count - x0));
    // the chunk's windows as ordinary records (windows overlap; the record checks want monotone offsets)
    for (uint32_t x = 0; x < m; x++) {
      const uint64_t s = wp.start(first + x0 + x);
      std::memcpy(cb.data() + static_cast<uint64_t>(x) * w, bases + s, w);
      if (constraint) std::memcpy(cc.data() + static_cast<uint64_t>(x) * w, constraint + s, w);
      offs[x] = static_cast<uint64_t>(x) * w;
    }
    offs[m] = static_cast<uint64_t>(m) * w;
    ConsCall cons;
    if (int rc = cons.prepare(m, offs.data(), constraint ? cc.data() : nullptr, wp.band)) return rc;
    StagedCall sc(c, true);
    if (int rc = sc.stage(c, "rnamc_bpp_windowed", m, cb.data(), offs.data(), cons)) return rc;
    uint64_t launches = 0;  // (run_batch* resets the context's statistics when it starts)
    size_t ev_pairs = 0;
    GroupHooks hooks;
    // (the group's triangles stay on the device, at group-local offsets)
    hooks.before = [&](size_t g, float** out_base) -> int {
      if (g == 0) {
        // the plan of the chunk is cut: one item per record for all its groups, uploaded once (the
        // host copy lives until the chunk's stream is drained)
        for (size_t x = 0; x < c->descs.size(); x++) {
          const SeqDesc& sd = c->descs[x];
          items[x].bpp_off = sd.out_off;
          items[x].start = wp.start(first + x0 + sd.batch_idx);
        }
        HIPCHK(grow_device(reinterpret_cast<void**>(&c->wn_items), &c->wn_items_cap,
                           static_cast<uint64_t>(m) * sizeof(WindowItem)));
        HIPCHK(hipMemcpyAsync(c->wn_items, items.data(), static_cast<uint64_t>(m) * sizeof(WindowItem),
                              hipMemcpyHostToDevice, st));
        if (prof)
          if (int rc = event_pairs(&c->wn_events, c->group_begin.size() - 1)) return rc;
      }
      return group_triangles(c, g, out_base);
    };
    hooks.after = [&](size_t g, uint32_t first_desc, uint32_t n_desc) -> int {
      // the group's finalize kernel is enqueued on `st`; the next group's writes st_out[0] behind
      // these launches in stream order: no host round-trip
      if (prof) HIPCHK(hipEventRecord(c->wn_events[2 * g], st));
      for (uint32_t x = 0; x < n_desc; x += 65535u) {
        launch_window_accumulate(c->wn_items + first_desc + x, std::min(n_desc - x, 65535u), c->st_out[0], w,
                                 wp.band, wp.n, c->wn_sum, c->wn_cnt, st);
        launches++;
      }
      HIPCHK(hipGetLastError());
      if (prof) {
        HIPCHK(hipEventRecord(c->wn_events[2 * g + 1], st));
        ev_pairs = g + 1;
      }
      return RNAMC_OK;
    };
    int rc = run_batch_mode(c, m, c->st_bases, sc.doff.data(), uses_contra_model != 0, allows_short_hairpins != 0,
                            nullptr, nullptr, c->st_logz, st, sc.opts, &hooks);
    c->stats.launches_other += launches;
    c->stats.launches_window += launches;
    rc = sc.finish(c, rc, m, window_log_partition ? window_log_partition + first + x0 : nullptr);
    if (rc) return rc;
    if (prof)
      if (int rc2 = event_pairs_ms(c->wn_events, ev_pairs, &c->stats.ms_window)) return rc2;
    add_sweep_stats(&total, c->stats);
    total.launches_window += c->stats.launches_window;
    total.ms_window += c->stats.ms_window;
  }
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
    HIPCHK(grow_device(reinterpret_cast<void**>(&c->wn_sum), &c->wn_sum_cap, cells * sizeof(int64_t)));
    HIPCHK(grow_device(reinterpret_cast<void**>(&c->wn_cnt), &c->wn_cnt_cap, cells * sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(c->wn_sum, sum, cells * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->wn_cnt, cnt, cells * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  HIPCHK(grow_device(reinterpret_cast<void**>(&c->wn_band), &c->wn_band_cap, cells * sizeof(float)));
  if (paired_prob)
    HIPCHK(grow_device(reinterpret_cast<void**>(&c->wn_paired), &c->wn_paired_cap, wp.n * sizeof(float)));
  const bool prof = c->profile != 0;
  if (prof) {
    if (int rc = event_pairs(&c->wn_events, 1)) return rc;
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
  if (prof)
    if (int rc = event_pairs_ms(c->wn_events, 1, &c->stats.ms_window)) return rc;
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

// rnamc_ctx.cpp — life cycle of the device context behind the C ABI: create / destroy, parameter
// tables, knobs, the statistics of the last call, rnamc_debug_fetch.
#include "rnamc_ctx.h"

using namespace rnamc;

namespace rnamc {

int ensure_ws(rnamc_ctx* c, uint64_t floats) {
  if (c->ws_floats >= floats) return RNAMC_OK;
  if (c->d_ws) HIPCHK(hipDeviceSynchronize());  // earlier work may still use the old one
  c->ws_floats = 0;
  HIPCHK(c->d_ws.replace_exact(floats));
  c->ws_floats = floats;
  return RNAMC_OK;
}

}  // namespace rnamc

namespace {

int validate_params(const rnamc_params* params) {
  if (params->abi_version != RNAMC_ABI_VERSION || params->struct_bytes != sizeof(rnamc_params)) {
    set_last_error("rnamc_params header does not match this library's ABI");
    return RNAMC_ERR_INVALID_ARG;
  }
  const rnamc_turner_scores& t = params->turner;
  if (t.num_special_hairpins > RNAMC_MAX_SPECIAL_HAIRPINS ||
      t.max_hairpin_len_extrapolation > RNAMC_MAX_LOOP_LEN || t.min_hairpin_len_extrapolation < 2 ||
      t.min_hairpin_len_extrapolation - 1 > RNAMC_MAX_LOOP_LEN ||
      t.min_hairpin_len > t.max_hairpin_len_extrapolation) {
    set_last_error("Turner hairpin limits out of range");
    return RNAMC_ERR_INVALID_ARG;
  }
  return RNAMC_OK;
}

}  // namespace

extern "C" {

int rnamc_ctx_create(const rnamc_params* params, int device, uint64_t workspace_bytes,
                     rnamc_ctx** out) {
  if (!params || !out) return RNAMC_ERR_INVALID_ARG;
  *out = nullptr;
  if (int rc = validate_params(params)) return rc;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    set_last_error("no HIP device visible: librnamc has no CPU fallback");
    return RNAMC_ERR_NO_DEVICE;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) return RNAMC_ERR_NO_DEVICE;
  }
  if (device >= count) return RNAMC_ERR_INVALID_ARG;
  DeviceGuard guard(device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  rnamc_ctx* c = new (std::nothrow) rnamc_ctx();
  if (!c) return RNAMC_ERR_OOM;
  c->device = device;
  c->host_params = *params;
  auto fail = [&](int rc) {
    rnamc_ctx_destroy(c);
    return rc;
  };
  if (c->d_params.replace_exact(1) != hipSuccess) return fail(RNAMC_ERR_OOM);
  if (hipMemcpy(c->d_params, params, sizeof(rnamc_params), hipMemcpyHostToDevice) != hipSuccess)
    return fail(RNAMC_ERR_HIP);
  if (hipStreamCreateWithFlags(c->own_stream.put(), hipStreamNonBlocking) != hipSuccess)
    return fail(RNAMC_ERR_HIP);
  {
    // the pair-tail kernel carries the longest dependent chains of a diagonal: its few
    // workgroups should be placed first, the other kernel fills the rest of the chip
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(c->aux_stream.put(), hipStreamNonBlocking, hi) != hipSuccess)
      return fail(RNAMC_ERR_HIP);
#ifndef RNAMC_DBG_LAZY_BULK
    // the tree-order mode's side stream (mid-field products, lowest priority) is created HERE,
    // with the context, not at the first tree-order call: created as the process's fifth or later
    // stream (after the host entry's copy stream) it no longer gets a hardware queue of its own on
    // this runtime and its 100-600 us kernels sit in the queue of the sweep's 11 us launches
    // (measured: the n = 4096 tree-order sweep took 157 ms instead of 49.5 ms at the end of
    // bench.py's batch run)
    if (hipStreamCreateWithPriority(c->bulk_stream.put(), hipStreamNonBlocking, lo) != hipSuccess)
      return fail(RNAMC_ERR_HIP);
#endif
  }
  if (c->ev_a.grow(16) != hipSuccess || c->ev_b.grow(16) != hipSuccess) return fail(RNAMC_ERR_HIP);
  if (workspace_bytes) {
    int rc = ensure_ws(c, workspace_bytes / 4);
    if (rc) return fail(rc);
  }
  *out = c;
  return RNAMC_OK;
}

void rnamc_ctx_destroy(rnamc_ctx* c) {
  if (!c) return;
  DeviceGuard guard(c->device);
  (void)hipDeviceSynchronize();
  delete c;  // every member releases what it owns: with the context's device current, after the sync
}

int rnamc_ctx_set_params(rnamc_ctx* c, const rnamc_params* params) {
  if (!c || !params) return RNAMC_ERR_INVALID_ARG;
  if (int rc = validate_params(params)) return rc;
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  // work of earlier calls may still read the old tables
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(c->d_params, params, sizeof(rnamc_params), hipMemcpyHostToDevice));
  c->host_params = *params;
  c->tree_tabs_valid = false;
  c->hp_init_len = 0;  // the hairpin extrapolation table is derived from the Turner block
  c->fs_contra = c->fs_short = -1;
  c->fs_bases.clear();
  return RNAMC_OK;
}

int rnamc_ctx_set(rnamc_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  const std::string k(name);
  if (k == "summation_mode" && (value == 0 || value == 1)) {
    c->summation_mode = value;
  } else if (k == "tree_side_stream" && value >= 0 && value <= 2) {
    c->tree_side_force = value;
    c->side_probed = false;
  } else if (k == "tree_waves" && value >= 64) {
    c->tree_pol.waves = static_cast<uint64_t>(value);
  } else if (k == "tree_short" && value >= 1) {
    c->tree_pol.short_terms = static_cast<uint32_t>(std::min<int64_t>(value, 1 << 30));
  } else if (k == "tree_mid_wgs" && value >= 1) {
    c->tree_pol.mid_wgs = static_cast<uint32_t>(std::min<int64_t>(value, 1 << 20));
  } else if (k == "tree_ahead_waves" && value >= 0) {
    c->tree_pol.ahead_waves = static_cast<uint64_t>(value);
  } else if (k == "tree_dual" && (value == 0 || value == 1)) {
    c->tree_dual = value;
#ifdef RNAMC_GEN_DIAGS
  } else if (k == "tree_gen_batch" && value >= 1 && value <= RNAMC_GEN_DIAGS) {  // (experiments: see k_tlane_gen)
#else
  } else if (k == "tree_gen_batch" && value >= 1 && value <= 3) {
#endif
    c->tree_gen_batch = value;
  } else if (k == "tree_lane_band" && value >= 32 && value <= 128 && value % 32 == 0) {
    c->tree_lane_band = value;
  } else if (k == "tree_mid_mx" && (value == 0 || value == 1)) {
    c->tree_pol.mid_mx = static_cast<uint32_t>(value);
  } else if (k == "tree_lane" && value >= 0 && value <= 2) {
    c->tree_lane = value;
  } else if (k == "tree_mid_sync" && (value == 0 || value == 1)) {
    c->tree_mid_sync = value;
  } else if (k == "tree_lane_min_nt" && value >= 0) {
    c->tree_lane_min_nt = value;
  } else if (k == "tree_xcd_rows" && (value == 0 || value == 1)) {
    c->tree_pol.xcd_rows = static_cast<uint32_t>(value);
  } else if (k == "tree_ahead") {
    c->tree_ahead = value;
  } else if (k == "tree_two") {
    c->tree_two = value;
  } else if (k == "tree_band" && value >= 0 && value <= 128 && value % 32 == 0) {
    c->tree_band = value;
  } else if (k == "tree_tpc" && (value == 0 || value == 64 || value == 128 || value == 256 || value == 1024)) {
    c->tree_tpc = value;
  } else if (k == "group_max_seqs" && value >= 1) {
    c->group_max_seqs = std::min<int64_t>(value, 65535);
  } else if (k == "group_max_nt" && value >= 1) {
    c->group_max_nt = value;
  } else if (k == "group_ws_bytes" && value >= 4) {
    c->group_ws_bytes = value;
    c->group_ws_user = true;
  } else if (k == "centroid_chunk_bytes" && value >= 0) {
    c->centroid_chunk_bytes = value;
  } else if (k == "window_chunk_nt" && value >= 1) {
    c->window_chunk_nt = value;
  } else if (k == "mutant_chunk_nt" && value >= 1) {
    c->mutant_chunk_nt = value;
  } else if (k == "block_threads" && value >= 64 && value <= 256 && value % 64 == 0) {
    // (the sweep kernels are compiled with __launch_bounds__(256))
    c->block_threads = value;
  } else if (k == "profile") {
    c->profile = value;
  } else if (k == "order_inside" && value >= 0 && value <= 2) {
    c->order_inside = value;
  } else if (k == "order_outside" && value >= 0 && value <= 4) {
    c->order_outside = value;
  } else if (k == "dual_outside") {
    c->dual_outside = value;
  } else if (k == "dual_max_diag" && value >= 0) {
    c->dual_max_diag = value;
  } else if (k == "dual_min_cells" && value >= 0) {
    c->dual_min_cells = static_cast<uint64_t>(value);
  } else if (k == "fuse_inside") {
    c->fuse_inside = value;
  } else if (k == "latency_mode" && value >= 0 && value <= 2) {
    c->latency_mode = value;
  } else if (k == "lat_max_cells" && value >= 0) {
    c->lat_max_cells = value;
  } else if (k == "lat_inside" && (value == 0 || value == 2)) {
    c->lat_inside = value;
  } else if (k == "lat_split") {
    c->lat_split = value;
  } else if (k == "lat_merge") {
    c->lat_merge = value;
  } else if (k == "lat_zr_ahead") {
    c->lat_zr_ahead = value;
  } else if (k == "lat_e_waves" && value >= 0) {
    c->lat_e_waves = value;
  } else if (k == "lat_pairs") {
    c->lat_pairs = value;
#ifdef RNAMC_DEBUG_KNOBS  // result-changing: timing experiments only, never in a release build
  } else if (k == "debug_roles") {
    c->debug_roles = value;
  } else if (k == "tree_debug") {
    c->tree_debug = value;
#endif
  } else {
    return RNAMC_ERR_INVALID_ARG;
  }
  return RNAMC_OK;
}

int rnamc_ctx_last_stats(rnamc_ctx* c, rnamc_batch_stats* out) {
  if (!c || !out) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  *out = c->stats;
  return RNAMC_OK;
}

int rnamc_ctx_stats(rnamc_ctx* c, void* out, uint64_t out_bytes, uint64_t* lib_bytes) {
  if (!c || (!out && out_bytes)) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  if (lib_bytes) *lib_bytes = sizeof(rnamc_batch_stats);
  if (out && out_bytes)
    std::memcpy(out, &c->stats, static_cast<size_t>(std::min<uint64_t>(out_bytes, sizeof(rnamc_batch_stats))));
  return RNAMC_OK;
}

int rnamc_debug_fetch(rnamc_ctx* c, uint32_t seq_idx, int which, float* out_nxn) {
  if (!c || !out_nxn) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  if (c->group_begin.size() < 2) return RNAMC_ERR_INVALID_ARG;
  const size_t g = c->group_begin.size() - 2;
  const SeqDesc* sd = nullptr;
  for (uint32_t x = c->group_begin[g]; x < c->group_begin[g + 1]; x++)
    if (c->descs[x].batch_idx == seq_idx) sd = &c->descs[x];
  if (!sd) return RNAMC_ERR_INVALID_ARG;
  static const int kMat[7] = {M_QB, M_QA, M_Z, M_Q1D, M_MBC, M_PM, M_PM2};
  if (which < 0 || which > 6) return RNAMC_ERR_INVALID_ARG;
  const bool row_major = which >= 5;
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  HIPCHK(hipDeviceSynchronize());
  const uint32_t n = sd->n;
  std::vector<float> packed(sd->tri_pad);  // column-major slots are a little larger than tri
  // probs_multibranch{,2} live interleaved ({pm, pm2} per cell) in the two adjacent slots
  const uint64_t slot = row_major ? static_cast<uint64_t>(M_PM) : static_cast<uint64_t>(kMat[which]);
  const size_t count = static_cast<size_t>(sd->tri_pad) * (row_major ? 2 : 1);
  packed.resize(count);
  HIPCHK(hipMemcpy(packed.data(), c->d_ws + sd->ws_off + slot * sd->tri_pad, count * sizeof(float),
                   hipMemcpyDeviceToHost));
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (uint64_t x = 0; x < static_cast<uint64_t>(n) * n; x++) out_nxn[x] = nan;
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t j = i; j < n; j++) {
      const uint64_t d = j - i;
      const uint64_t cm = j >> 4, cr = j & 15u;
      const uint64_t idx = row_major ? 2ull * (16ull * (cm + 1ull) * (8ull * cm + cr) + i) + (which == 6 ? 1 : 0)
                                     : (d * n - d * (d - 1ull) / 2ull + i);
      // probs_multibranch{,2} exist from the outside sweep's lowest diagonal up: below it no launch form
      // writes the slot, which still holds the inside pass's M_ZRE / M_QM there (diagonal-major, another
      // layout).  Those cells are reported as the reference's "no entry", not as floats of another matrix.
      out_nxn[static_cast<uint64_t>(i) * n + j] =
          row_major && d < c->last_dmin_out ? -std::numeric_limits<float>::infinity() : packed[idx];
    }
  return RNAMC_OK;
}

int rnamc_debug_fetch_tree(rnamc_ctx* c, uint32_t seq_idx, int slot, float* out, uint64_t out_floats, uint32_t* ld,
                           uint64_t* floats) {
  if (!c || slot < 0 || slot >= rnamc::T_COUNT) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  // (h_tseqs is emptied when a call starts and filled by the tree-order sweep alone; one group: the
  // descriptors' offsets are relative to the workspace itself)
  if (c->group_begin.size() != 2 || c->h_tseqs.empty() || c->h_tseqs.size() != c->descs.size())
    return RNAMC_ERR_INVALID_ARG;
  const rnamc::TreeSeq* ts = nullptr;
  for (const rnamc::TreeSeq& t : c->h_tseqs)
    if (t.batch_idx == seq_idx) ts = &t;
  if (!ts) return RNAMC_ERR_INVALID_ARG;
  if (ld) *ld = ts->ld;
  if (floats) *floats = ts->msz;
  if (!out) return RNAMC_OK;
  if (out_floats < ts->msz) return RNAMC_ERR_INVALID_ARG;
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, c->d_ws + ts->ws_off + static_cast<uint64_t>(slot) * ts->msz, ts->msz * sizeof(float),
                   hipMemcpyDeviceToHost));
  return RNAMC_OK;
}

}  // extern "C"

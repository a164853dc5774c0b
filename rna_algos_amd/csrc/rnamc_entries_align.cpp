// rnamc_entries_align.cpp — rnamc_bpp_alignment: the rows of a multiple alignment, each without its
// gaps, through the bpp sweep group by group, and per group the integer accumulation of its
// device-resident triangles into the column-pair triangle of the alignment through the rows' column
// maps; then the average, the column profile and the consensus folds off the finished triangle
// (rnamc_align.hip).
#include "rnamc_entries.h"

using namespace rnamc;

namespace rnamc {

int bpp_alignment_check(uint32_t n_rows, uint32_t n_cols, const uint8_t* rows, const float* gammas, uint32_t ng,
                        const uint8_t* structs, const uint32_t* n_pairs, const float* expect_accuracy,
                        AlignRows* out) {
  if (!rows || n_rows == 0 || n_cols == 0 || n_rows > 65535u || n_cols > RNAMC_MAX_SEQ_LEN) {
    set_last_error("rnamc_bpp_alignment: rows must be given, n_rows and n_cols 1 .. 65535");
    return RNAMC_ERR_INVALID_ARG;
  }
  if (ng > 65535u || (ng != 0 && !gammas)) return RNAMC_ERR_INVALID_ARG;
  if (ng == 0 && (structs || n_pairs || expect_accuracy)) {
    set_last_error("rnamc_bpp_alignment: structures need thresholds");
    return RNAMC_ERR_INVALID_ARG;
  }
  try {  // nothing may throw across the C boundary
    out->n_cols = n_cols;
    out->offsets.assign(1, 0);
    out->offsets.reserve(static_cast<size_t>(n_rows) + 1);
    out->row_idx.reserve(n_rows);
    for (uint32_t s = 0; s < n_rows; s++) {
      const uint8_t* row = rows + static_cast<uint64_t>(s) * n_cols;
      for (uint32_t col = 0; col < n_cols; col++) {
        if (row[col] > 4) {
          set_last_error("rnamc_bpp_alignment: row " + std::to_string(s) + ", column " + std::to_string(col) +
                         ": code " + std::to_string(row[col]) + " (0 .. 3 a base, 4 a gap)");
          return RNAMC_ERR_INVALID_BASE;
        }
        if (row[col] == 4) continue;
        out->bases.push_back(row[col]);
        out->maps.push_back(col);
      }
      if (out->bases.size() == out->offsets.back()) {
        set_last_error("rnamc_bpp_alignment: row " + std::to_string(s) + " has no base");
        return RNAMC_ERR_EMPTY_SEQ;
      }
      out->offsets.push_back(out->bases.size());
      out->row_idx.push_back(s);
    }
  } catch (const std::exception&) {
    set_last_error("rnamc_bpp_alignment: no host memory");
    return RNAMC_ERR_OOM;
  }
  return check_records(n_rows, out->bases.data(), out->offsets.data());
}

int bpp_alignment_accumulate(rnamc_ctx* c, const AlignRows& ar, uint32_t max_bp_span, int uses_contra_model,
                             int allows_short_hairpins, float* log_partition) {
  const uint32_t n = static_cast<uint32_t>(ar.row_idx.size());
  const uint64_t cells = rnamc_bpp_len(ar.n_cols);
  ConsCall cons;
  if (int rc = cons.prepare(n, ar.offsets.data(), nullptr, max_bp_span)) return rc;
  std::vector<AlignItem> items;  // (the host copies live until the call's stream is drained)
  std::vector<float> h_logz;
  try {  // nothing may throw across the C boundary
    items.resize(n);
    h_logz.resize(n);
  } catch (const std::exception&) {
    set_last_error("rnamc_bpp_alignment: no host memory");
    return RNAMC_ERR_OOM;
  }
  StagedCall sc(c, true);
  if (int rc = sc.stage(c, "rnamc_bpp_alignment", n, ar.bases.data(), ar.offsets.data(), cons)) return rc;
  hipStream_t st = c->own_stream;  // (a call with hooks never takes the two-stream route of the tree order)
  HIPCHK(c->al_sum.grow(cells));
  HIPCHK(c->al_cnt.grow(cells));
  HIPCHK(c->al_items.grow(n));
  // once per call, not per group
  HIPCHK(hipMemsetAsync(c->al_sum, 0, cells * sizeof(int64_t), st));
  HIPCHK(hipMemsetAsync(c->al_cnt, 0, cells * sizeof(uint32_t), st));
  HIPCHK(c->al_maps.upload(ar.maps.data(), ar.maps.size(), st));
  uint64_t launches = 0;  // (run_batch* resets the context's statistics when it starts)
  GroupHooks hooks;
  hooks.before = [&](size_t g, float** out_base) -> int {
    if (g == 0) {
      // the plan of the call is cut: one item per row for all its groups, uploaded once
      for (size_t x = 0; x < c->descs.size(); x++) {
        const SeqDesc& sd = c->descs[x];
        items[x].bpp_off = sd.out_off;
        items[x].map_off = ar.offsets[sd.batch_idx];
        items[x].n = sd.n;
        items[x].pad_ = 0;
      }
      HIPCHK(hipMemcpyAsync(c->al_items, items.data(), n * sizeof(AlignItem), hipMemcpyHostToDevice, st));
    }
    return group_triangles(c, g, out_base);
  };
  hooks.after = [&](size_t, uint32_t first, uint32_t count) -> int {
    // the group's finalize kernel is enqueued on `st`; the next group's writes st_out[0] behind these
    // launches in stream order.  Rows longest first: the first item of a launch has the most cells
    for (uint32_t x = 0; x < count; x += 65535u) {
      launch_align_accumulate(c->al_items + first + x, std::min(count - x, 65535u), items[first + x].n, c->st_out[0],
                              c->al_maps, ar.n_cols, c->al_sum, c->al_cnt, st);
      launches++;
    }
    HIPCHK(hipGetLastError());
    return RNAMC_OK;
  };
  int rc = run_batch_mode(c, n, c->st_bases, sc.doff.data(), uses_contra_model != 0, allows_short_hairpins != 0,
                          nullptr, nullptr, c->st_logz, st, sc.opts, &hooks);
  c->stats.launches_other += launches;
  rc = sc.finish(c, rc, n, log_partition ? h_logz.data() : nullptr);
  if (rc) return rc;
  if (log_partition)
    for (uint32_t s = 0; s < n; s++) log_partition[ar.row_idx[s]] = h_logz[s];
  return RNAMC_OK;
}

int bpp_alignment_fetch(rnamc_ctx* c, uint32_t n_cols, int64_t* sum, uint32_t* cnt) {
  const uint64_t cells = rnamc_bpp_len(n_cols);
  HIPCHK(hipMemcpyAsync(sum, c->al_sum, cells * sizeof(int64_t), hipMemcpyDeviceToHost, c->own_stream));
  HIPCHK(hipMemcpyAsync(cnt, c->al_cnt, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->own_stream));
  HIPCHK(hipStreamSynchronize(c->own_stream));
  return RNAMC_OK;
}

int bpp_alignment_finish(rnamc_ctx* c, uint32_t n_rows, uint32_t n_cols, const int64_t* sum, const uint32_t* cnt,
                         const float* gammas, uint32_t ng, float* bpp, float* col_paired, uint8_t* structs,
                         uint32_t* n_pairs, float* expect_accuracy) {
  hipStream_t st = c->own_stream;
  const uint64_t cells = rnamc_bpp_len(n_cols);
  const bool folds = ng != 0 && (structs || n_pairs || expect_accuracy);
  if (sum) {  // the totals of a pool's shards
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(c->al_sum.grow(cells));
    HIPCHK(c->al_cnt.grow(cells));
    HIPCHK(hipMemcpyAsync(c->al_sum, sum, cells * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->al_cnt, cnt, cells * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  uint64_t launches = 0;
  if (bpp || folds) {
    HIPCHK(c->al_out.grow(cells));
    launch_align_finalize(n_cols, n_rows, c->al_sum, c->al_cnt, c->al_out, st);
    launches++;
  }
  if (col_paired) {
    HIPCHK(c->al_paired.grow(n_cols));
    launch_align_paired(n_cols, n_rows, c->al_sum, c->al_cnt, c->al_paired, st);
    launches++;
  }
  HIPCHK(hipGetLastError());
  if (bpp) HIPCHK(hipMemcpyAsync(bpp, c->al_out, cells * sizeof(float), hipMemcpyDeviceToHost, st));
  if (col_paired)
    HIPCHK(hipMemcpyAsync(col_paired, c->al_paired, n_cols * sizeof(float), hipMemcpyDeviceToHost, st));
  if (folds) {
    // the sweeps are through: the workspace holds the (max,+) triangles of the thresholds, one item
    // of n_cols columns each (the rows were shorter: it may have to grow)
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = ensure_ws(c, centroid_item_floats(n_cols))) return rc;
    CentroidStage stage;
    if (int rc = stage.init(c, "rnamc_bpp_alignment")) return rc;
    const CentroidSeq seq{0, n_cols};
    const int rc = stage.run(c, c->al_out, &seq, 1, gammas, ng,
                             [&](uint32_t, uint32_t gi, const uint8_t* row, uint32_t np, float acc) {
                               if (structs) {
                                 uint8_t* to = structs + static_cast<uint64_t>(gi) * n_cols;
                                 if (row) std::memcpy(to, row, n_cols); else std::memset(to, '.', n_cols);
                               }
                               if (n_pairs) n_pairs[gi] = np;
                               if (expect_accuracy) expect_accuracy[gi] = acc;
                             });
    if (rc) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    launches += stage.launches;
  }
  HIPCHK(hipStreamSynchronize(st));
  c->stats.launches_other += launches;
  return RNAMC_OK;
}

}  // namespace rnamc

extern "C" {

int rnamc_bpp_alignment(rnamc_ctx* c, uint32_t n_rows, uint32_t n_cols, const uint8_t* rows, uint32_t max_bp_span,
                        int uses_contra_model, int allows_short_hairpins, const float* centroid_thresholds,
                        uint32_t n_thresholds, float* bpp, float* col_paired, uint8_t* structs, uint32_t* n_pairs,
                        float* expect_accuracy, float* log_partition, uint32_t* row_len) {
  if (!c) return RNAMC_ERR_INVALID_ARG;
  AlignRows ar;
  if (int rc = bpp_alignment_check(n_rows, n_cols, rows, centroid_thresholds, n_thresholds, structs, n_pairs,
                                   expect_accuracy, &ar))
    return rc;
  if (row_len)
    for (uint32_t s = 0; s < n_rows; s++) row_len[s] = static_cast<uint32_t>(ar.offsets[s + 1] - ar.offsets[s]);
  std::unique_lock<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  if (int rc = bpp_alignment_accumulate(c, ar, max_bp_span, uses_contra_model, allows_short_hairpins,
                                        log_partition)) {
    (void)hipStreamSynchronize(c->own_stream);
    return rc;
  }
  return bpp_alignment_finish(c, n_rows, n_cols, nullptr, nullptr, centroid_thresholds, n_thresholds, bpp,
                              col_paired, structs, n_pairs, expect_accuracy);
}

}  // extern "C"

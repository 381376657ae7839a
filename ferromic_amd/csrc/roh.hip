// roh.hip — runs of homozygosity: fmh_roh_scan (per sample the qualifying runs of the PLINK-style sliding-window scan along the kept rows,
// exact integers from the bit planes: a scan kernel over (row block, sample group) items that leaves one record per (block, sample), and a
// stitch kernel that joins the blocks), its host twin fmh_roh_scan_host, and the host-only fmh_roh_need and fmh_roh_sort_segments.  Kernels
// in roh_kernels.hpp, host arithmetic in roh_host.hpp, what it shares with the IBD segments in segment_*.hpp; definition in
// include/ferromic_hip.h, scheme in DESIGN.md section 3.21.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "abi_internal.hpp"
#include "roh_host.hpp"
#include "roh_kernels.hpp"
#include "segment_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;

namespace {

const fmh_roh_out kRohNoTables{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

bool any_table(const fmh_roh_out& o) { return o.d_n_runs || o.d_sum_sites || o.d_sum_length || o.d_longest_length || o.d_bin_runs || o.d_bin_length; }

int check_roh_params(const fmh_roh_params& p) {
  if (const char* refused = roh_check_params(p)) return fail(FMH_ERR_INVALID, "%s (window %u, n_bins %u)", refused, p.window, p.n_bins);
  return FMH_OK;
}

}  // namespace

extern "C" int fmh_roh_scan(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                            const uint8_t* h_keep_or_null, const uint32_t* h_positions_or_null, const fmh_roh_params* params,
                            const fmh_roh_out* out_or_null, fmh_roh_segment* d_segments_or_null, size_t segment_capacity, uint64_t* h_segment_count,
                            void* stream) {
  // ---- every refusal, before any launch ----
  const fmh_roh_out out = out_or_null ? *out_or_null : kRohNoTables;
  FMH_TRY(check_segment_scan(m, params, h_samples_or_null, n_samples, row_begin, row_count, h_positions_or_null, any_table(out), d_segments_or_null,
                             h_segment_count, "runs of homozygosity", [&] { return check_roh_params(*params); }));
  const fmh_roh_params& P = *params;

  // ---- the kept rows, their positions and breaks ----
  const size_t n = n_samples, W = P.window, nb = P.n_bins;
  SegmentFrame frame(h_keep_or_null, h_positions_or_null, row_begin, row_count, h_samples_or_null, n);
  const size_t K = frame.kept.rows.size();
  const bool segments = d_segments_or_null || h_segment_count;
  const size_t capacity = d_segments_or_null ? segment_capacity : 0;

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  if (h_segment_count) *h_segment_count = 0;
  if (K < W) {  // no window, no run (K == 0 included): zero tables
    FMH_TRY(call.start());
    for (unsigned long long* t : {out.d_n_runs, out.d_sum_sites, out.d_sum_length, out.d_longest_length})
      if (t) HIP_TRY(hipMemsetAsync(t, 0, n * sizeof(unsigned long long), st));
    for (unsigned long long* t : {out.d_bin_runs, out.d_bin_length})
      if (t && nb) HIP_TRY(hipMemsetAsync(t, 0, n * nb * sizeof(unsigned long long), st));
    return call.finish();
  }

  const std::vector<unsigned long long> brk = break_bitmap(frame.kept.x, P.max_gap, kRohBreakOffset, roh_break_words(K, W));
  const uint32_t groups = frame.groups;
  const size_t spad = frame.rank.size();

  const size_t item_rows = roh_item_rows(options().roh_item_rows.load(std::memory_order_relaxed));
  const size_t n_blocks = (K + item_rows - 1) / item_rows;
  FMH_TRY(check_item_count(n_blocks * groups, "FMH_ROH_ITEM_ROWS"));

  uint32_t *d_samples = nullptr, *rec32 = nullptr;
  unsigned long long* rec64 = nullptr;
  FMH_TRY(frame.upload(call, m, brk, segments));
  if (h_samples_or_null) FMH_TRY(call.upload(h_samples_or_null, n, &d_samples));
  FMH_TRY(call.scratch.get(&rec32, n_blocks * RohRec::n32 * spad));
  FMH_TRY(call.scratch.get(&rec64, n_blocks * (kRohRec64 + 2 * nb) * spad));

  RohArgs a{};
  set_plane_rows(a, m);
  a.nvec = frame.nvec;
  a.groups = groups;
  a.row_begin = row_begin;
  a.rows = frame.d_rows;
  a.flags = frame.d_flags;
  a.x = frame.d_x;
  a.brk = frame.d_brk;
  a.rank = frame.d_rank;
  a.samples = d_samples;
  a.n = (uint32_t)n;
  a.K = (uint32_t)K;
  a.item_rows = (uint32_t)item_rows;
  a.n_blocks = (uint32_t)n_blocks;
  a.n_items = (uint32_t)(n_blocks * groups);
  a.P = P;
  a.rec32 = rec32;
  a.rec64 = rec64;
  a.segments = d_segments_or_null;
  a.capacity = capacity;
  a.counter = frame.d_counter;
  a.out = out;

  FMH_TRY(call.start());
  FMH_TRY(frame.launch_flags(call, m, row_begin));
  {
    const size_t lds = 2 * kRohStepRows * 4 * sizeof(uint4) + 65 * sizeof(uint32_t);
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(roh_scan_kernel), kRohThreads, 0, a.n_items, call.ws->cus, &grid, lds));
    hipLaunchKernelGGL(roh_scan_kernel, dim3((unsigned)grid), dim3(kRohThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(roh_stitch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return frame.finish(call, h_segment_count);
}

// ---- host only (no device) -------------------------------------------------------------------------------------------------------------------
extern "C" int fmh_roh_scan_host(const uint8_t* h_state, const uint32_t* h_x_or_null, size_t n_kept, size_t n_samples, const fmh_roh_params* params,
                                 const fmh_roh_out* out_or_null, fmh_roh_segment* h_segments_or_null, size_t segment_capacity,
                                 uint64_t* h_segment_count) {
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (n_kept != 0 && !h_state) return fail(FMH_ERR_INVALID, "NULL state");
  const fmh_roh_out out = out_or_null ? *out_or_null : kRohNoTables;
  FMH_TRY(check_roh_params(*params));
  FMH_TRY(check_segment_request(h_x_or_null, n_kept, any_table(out), h_segments_or_null, h_segment_count));
  if (n_kept >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "%zu kept rows: fewer than 2^32 - 1 are taken", n_kept);
  for (size_t i = 0; i < n_kept * n_samples; ++i)
    if (h_state[i] > 2) return fail(FMH_ERR_INVALID, "state %u (kept row %zu, sample %zu) is not 0, 1 or 2", h_state[i], i / n_samples, i % n_samples);
  roh_scan_host(h_state, h_x_or_null, n_kept, n_samples, *params, out, h_segments_or_null, h_segments_or_null ? segment_capacity : 0, h_segment_count);
  return FMH_OK;
}

extern "C" int fmh_roh_need(double threshold, uint32_t window, uint8_t* need) {
  if (const char* refused = roh_need(threshold, window, need)) return fail(FMH_ERR_INVALID, "%s (threshold %g, window %u)", refused, threshold, window);
  return FMH_OK;
}

extern "C" int fmh_roh_sort_segments(fmh_roh_segment* h_segments, size_t count) {
  if (count != 0 && !h_segments) return fail(FMH_ERR_INVALID, "NULL segments");
  std::sort(h_segments, h_segments + count, roh_segment_less);
  return FMH_OK;
}

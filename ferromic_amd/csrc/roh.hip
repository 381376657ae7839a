// roh.hip — runs of homozygosity: fmh_roh_scan (per sample the qualifying runs of the PLINK-style sliding-window scan along the kept rows,
// exact integers from the bit planes: a scan kernel over (row block, sample group) items that leaves one record per (block, sample), and a
// stitch kernel that joins the blocks), its host twin fmh_roh_scan_host, and the host-only fmh_roh_need and fmh_roh_sort_segments.  Kernels
// in roh_kernels.hpp, host arithmetic in roh_host.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.21.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "abi_internal.hpp"
#include "roh_host.hpp"
#include "roh_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;

namespace {

const fmh_roh_out kRohNoTables{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

bool any_table(const fmh_roh_out& o) { return o.d_n_runs || o.d_sum_sites || o.d_sum_length || o.d_longest_length || o.d_bin_runs || o.d_bin_length; }

// what the two entry points refuse alike, in the header's order, from the window on
int check_roh_request(const fmh_roh_params& p, const uint32_t* x, size_t x_count, const fmh_roh_out& out, const void* segments, const uint64_t* count) {
  if (const char* refused = roh_check_params(p)) return fail(FMH_ERR_INVALID, "%s (window %u, n_bins %u)", refused, p.window, p.n_bins);
  for (size_t k = 1; x && k < x_count; ++k)
    if (x[k] < x[k - 1]) return fail(FMH_ERR_INVALID, "the positions descend at row entry %zu of the range", k);
  if (!any_table(out) && !segments && !count) return fail(FMH_ERR_INVALID, "every output is NULL");
  if (segments && !count) return fail(FMH_ERR_INVALID, "a segment buffer is given but h_segment_count is NULL");
  return FMH_OK;
}

}  // namespace

extern "C" int fmh_roh_scan(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                            const uint8_t* h_keep_or_null, const uint32_t* h_positions_or_null, const fmh_roh_params* params,
                            const fmh_roh_out* out_or_null, fmh_roh_segment* d_segments_or_null, size_t segment_capacity, uint64_t* h_segment_count,
                            void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  const fmh_roh_params& P = *params;
  const fmh_roh_out out = out_or_null ? *out_or_null : kRohNoTables;
  FMH_TRY(check_roh_request(P, h_positions_or_null ? h_positions_or_null + row_begin : nullptr, row_count, out, d_segments_or_null, h_segment_count));
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "runs of homozygosity take diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_packed(m, "runs of homozygosity read"));
  if (row_count >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "a range of %zu rows: fewer than 2^32 - 1 are taken (split the rows)", row_count);

  // ---- the kept rows, their positions and breaks ----
  const size_t n = n_samples, W = P.window, nb = P.n_bins;
  std::vector<uint32_t> rows, x;
  rows.reserve(row_count);
  for (size_t r = 0; r < row_count; ++r)
    if (!h_keep_or_null || h_keep_or_null[r]) rows.push_back((uint32_t)r);
  const size_t K = rows.size();
  x.resize(K);
  for (size_t k = 0; k < K; ++k) x[k] = h_positions_or_null ? h_positions_or_null[row_begin + rows[k]] : rows[k];
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

  std::vector<unsigned long long> brk((K + 64 + 2 * W + 63) / 64 + 2, 0ull);  // bit k + 64
  if (P.max_gap > 0)
    for (size_t k = 1; k < K; ++k)
      if (x[k] - x[k - 1] > P.max_gap) brk[(k + 64) >> 6] |= 1ull << ((k + 64) & 63);

  const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
  const uint32_t nvec = last / 64 + 1;  // 64 samples per 16 bytes of a row; within the row: sample `last` exists
  const uint32_t groups = (nvec + 3) / 4;
  const size_t spad = (size_t)groups * kRohGroupSamples;
  std::vector<uint32_t> rank(spad, kRohNone);
  for (size_t i = 0; i < n; ++i) rank[h_samples_or_null ? h_samples_or_null[i] : i] = (uint32_t)i;

  const size_t item_rows = roh_item_rows(options().roh_item_rows.load(std::memory_order_relaxed));
  const size_t n_blocks = (K + item_rows - 1) / item_rows;
  FMH_TRY(check_item_count(n_blocks * groups, "FMH_ROH_ITEM_ROWS"));

  uint32_t *d_rows = nullptr, *d_x = nullptr, *d_rank = nullptr, *d_samples = nullptr, *rec32 = nullptr;
  unsigned long long *d_brk = nullptr, *rec64 = nullptr, *d_counter = nullptr;
  uint8_t* d_flags = nullptr;
  FMH_TRY(call.upload(rows.data(), K, &d_rows));
  FMH_TRY(call.upload(x.data(), K, &d_x));
  FMH_TRY(call.upload(brk.data(), brk.size(), &d_brk));
  FMH_TRY(call.upload(rank.data(), spad, &d_rank));
  if (h_samples_or_null) FMH_TRY(call.upload(h_samples_or_null, n, &d_samples));
  FMH_TRY(call.scratch.get(&rec32, n_blocks * kRohRec32 * spad));
  FMH_TRY(call.scratch.get(&rec64, n_blocks * (kRohRec64 + 2 * nb) * spad));
  if (segments) FMH_TRY(call.zeroed(1, &d_counter));
  const bool any_flag = m->pc || m->p1 || m->p2;
  if (any_flag) FMH_TRY(call.scratch.get(&d_flags, K));

  RohArgs a{};
  set_plane_rows(a, m);
  a.nvec = nvec;
  a.groups = groups;
  a.row_begin = row_begin;
  a.rows = d_rows;
  a.flags = d_flags;
  a.x = d_x;
  a.brk = d_brk;
  a.rank = d_rank;
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
  a.counter = d_counter;
  a.out = out;

  FMH_TRY(call.start());
  if (any_flag) {
    PlaneRows planes{};
    set_plane_rows(planes, m);
    hipLaunchKernelGGL(roh_flags_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, planes, row_begin, d_rows, (uint32_t)K, d_flags);
    HIP_TRY(hipGetLastError());
  }
  {
    const size_t lds = 2 * kRohStepRows * 4 * sizeof(uint4) + 65 * sizeof(uint32_t);
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(roh_scan_kernel), kRohThreads, 0, a.n_items, call.ws->cus, &grid, lds));
    hipLaunchKernelGGL(roh_scan_kernel, dim3((unsigned)grid), dim3(kRohThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(roh_stitch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  FMH_TRY(call.stop());
  unsigned long long count = 0;
  if (segments) HIP_TRY(hipMemcpyAsync(&count, d_counter, sizeof count, hipMemcpyDeviceToHost, st));
  FMH_TRY(call.finish());
  if (h_segment_count) *h_segment_count = count;
  return FMH_OK;
}

// ---- host only (no device) -------------------------------------------------------------------------------------------------------------------
extern "C" int fmh_roh_scan_host(const uint8_t* h_state, const uint32_t* h_x_or_null, size_t n_kept, size_t n_samples, const fmh_roh_params* params,
                                 const fmh_roh_out* out_or_null, fmh_roh_segment* h_segments_or_null, size_t segment_capacity,
                                 uint64_t* h_segment_count) {
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (n_kept != 0 && !h_state) return fail(FMH_ERR_INVALID, "NULL state");
  const fmh_roh_out out = out_or_null ? *out_or_null : kRohNoTables;
  FMH_TRY(check_roh_request(*params, h_x_or_null, n_kept, out, h_segments_or_null, h_segment_count));
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
